// Lean sweep kernel variants (stencil_tbl_impl.hpp launch_tbl) without source or
// walls: H3D_V(Real, R, WY, K, Q, NTS, SW, PART).  PART (0-3) names the
// stencil_tbl_partN.hip unit that instantiates the variant, so that the heavy
// kernel instantiations compile in parallel.  The dispatch is this list
// (stencil_tbl.hip hands it, as types, to stencil_tbl_form.hpp dispatch_tbl_form):
// a spec resolving to a line's R, WY, K, Q and store field NTS (spec field 7:
// 2 = nt, 1 / 16 = sc0 / sc1, 64 = last residual only) launches that line, and
// any other spec is an error.  (tests/test_lean_variants_cpu.py walks the specs
// in both directions; tests/test_gpu_lean_variants.py launches every entry, so a
// new entry is tested by being listed.)  A variant
// whose kernel needs scratch is refused by launch_tbl and so is not listed: in
// fp64 that leaves out (R, WY, K, Q) = (3,16,4,3|4), (2,16,5,3), (4,12,4,3|4),
// (4,12,5,3) and the every-residual forms of (4,12,4,3) and (3,12,5,3), in fp32
// (3,16,6,3), (4,16,5,3) and (4,16,6,3), which spill 28-236 B per lane.
// Registers: 16 waves (<= 128 VGPRs, LDS 2K x 16 KiB) reach K <= 4 in fp64, 12
// waves (<= 168 VGPRs) K = 5; 8 waves (<= 256 VGPRs, 2 per SIMD) carry the
// 48-row tiles at K = 4 and the fp64 K = 5 / 6 defaults.  The fp64 48-row K = 4
// and 36-row K = 5 tiles of 12 waves take 167 VGPRs without the K - 1 residual
// maxima, so they exist with the last residual only (NTS 66).  fp32 has half
// the registers and LDS per row, so deeper sweeps fit 16 waves and the taller
// tiles 12: the fp32-only lines (in fp64 each of these shapes spills: not built).
// (3,16,3,3,66) is the fp64 / fp32 K = 3 default with the last residual only,
// (3,12,4,3,2) the fp64 K = 4 default of long sweeps (12 waves, 36 rows); the
// K = 2 lines are the partial sweeps' candidates.
// thin x slabs (y-marching, SW: picked by box shape, kernels.hpp lean_thin_slab),
// store-policy variants of the default shapes, then the
// shapes selectable through the kernel spec; fp32-only entries last.
// H3D_VE(Real, R, WY, K, Q, NTS, SW, EW, PART): the variants with the edge role
// (spec field 9 = EW = 1 + E: the two halo waves of a tile evaluate only the
// stages inside its cone and own E more rows each).  fp64 K = 4, 12 waves of 4
// rows, last residual only: 48-row tiles storing 40 rows (E = 0) and 52-row
// tiles storing 44 (E = 2).
H3D_V(double, 2, 5, 3, 3, 2, true, 2)
H3D_V(double, 3, 3, 3, 3, 2, true, 3)
H3D_V(double, 3, 4, 4, 3, 2, true, 2)
H3D_V(double, 3, 16, 3, 3, 2, false, 0)
H3D_V(double, 3, 16, 3, 3, 66, false, 1)
H3D_V(double, 3, 16, 3, 3, 3, false, 1)
H3D_V(double, 3, 16, 3, 3, 17, false, 2)
H3D_V(double, 3, 16, 3, 3, 18, false, 0)
H3D_V(double, 3, 16, 3, 3, 19, false, 3)
H3D_V(double, 2, 16, 4, 3, 2, false, 3)
H3D_V(double, 3, 16, 2, 3, 2, false, 1)
H3D_V(double, 3, 16, 2, 3, 66, false, 3)
H3D_V(double, 5, 16, 2, 3, 2, false, 2)
H3D_V(double, 5, 16, 2, 3, 66, false, 0)
H3D_V(double, 3, 12, 4, 3, 2, false, 0)
H3D_V(double, 3, 12, 4, 3, 66, false, 1)
H3D_V(double, 4, 12, 4, 3, 66, false, 3)
H3D_V(double, 3, 12, 5, 3, 66, false, 0)
H3D_VE(double, 4, 12, 4, 3, 66, false, 1, 1)
H3D_VE(double, 4, 12, 4, 3, 66, false, 3, 2)
H3D_V(double, 3, 16, 3, 3, 0, false, 1)
H3D_V(double, 3, 16, 3, 4, 0, false, 2)
H3D_V(double, 2, 16, 4, 3, 0, false, 1)
H3D_V(double, 2, 16, 4, 4, 0, false, 3)
H3D_V(double, 2, 16, 3, 3, 0, false, 3)
H3D_V(double, 2, 16, 4, 6, 0, false, 2)
H3D_V(double, 2, 16, 3, 6, 0, false, 2)
H3D_V(double, 3, 16, 3, 6, 0, false, 0)
H3D_V(double, 2, 16, 2, 6, 0, false, 0)
H3D_V(double, 3, 16, 2, 3, 0, false, 0)
H3D_V(double, 2, 16, 2, 3, 0, false, 1)
H3D_V(double, 3, 12, 4, 3, 0, false, 3)
H3D_V(double, 6, 8, 4, 3, 0, false, 1)
H3D_V(double, 6, 8, 3, 3, 0, false, 1)
H3D_V(double, 6, 8, 4, 4, 0, false, 2)
H3D_V(double, 5, 8, 4, 3, 0, false, 3)
H3D_V(double, 3, 8, 5, 3, 0, false, 1)
H3D_V(double, 3, 8, 6, 3, 0, false, 2)
H3D_V(float, 2, 5, 3, 3, 0, true, 1)
H3D_V(float, 3, 3, 3, 3, 0, true, 3)
H3D_V(float, 3, 4, 4, 3, 0, true, 1)
H3D_V(float, 3, 16, 3, 3, 2, false, 3)
H3D_V(float, 3, 16, 3, 3, 66, false, 2)
H3D_V(float, 3, 16, 3, 3, 3, false, 0)
H3D_V(float, 3, 16, 3, 3, 17, false, 2)
H3D_V(float, 3, 16, 3, 3, 18, false, 3)
H3D_V(float, 3, 16, 3, 3, 19, false, 0)
H3D_V(float, 2, 16, 4, 3, 2, false, 0)
H3D_V(float, 3, 16, 2, 3, 2, false, 3)
H3D_V(float, 3, 16, 2, 3, 66, false, 0)
H3D_V(float, 5, 16, 2, 3, 2, false, 0)
H3D_V(float, 5, 16, 2, 3, 66, false, 3)
H3D_V(float, 3, 12, 4, 3, 2, false, 0)
H3D_V(float, 3, 12, 4, 3, 66, false, 2)
H3D_V(float, 4, 12, 4, 3, 2, false, 3)
H3D_V(float, 3, 16, 4, 3, 0, false, 1)
H3D_V(float, 3, 16, 4, 4, 0, false, 2)
H3D_V(float, 3, 16, 3, 3, 0, false, 2)
H3D_V(float, 3, 16, 3, 4, 0, false, 1)
H3D_V(float, 2, 16, 4, 3, 0, false, 2)
H3D_V(float, 2, 16, 4, 4, 0, false, 1)
H3D_V(float, 2, 16, 5, 3, 0, false, 1)
H3D_V(float, 2, 16, 3, 3, 0, false, 1)
H3D_V(float, 2, 16, 4, 6, 0, false, 0)
H3D_V(float, 2, 16, 3, 6, 0, false, 3)
H3D_V(float, 3, 16, 3, 6, 0, false, 3)
H3D_V(float, 2, 16, 2, 6, 0, false, 3)
H3D_V(float, 3, 16, 2, 3, 0, false, 2)
H3D_V(float, 2, 16, 2, 3, 0, false, 0)
H3D_V(float, 4, 12, 4, 3, 0, false, 2)
H3D_V(float, 4, 12, 4, 4, 0, false, 0)
H3D_V(float, 4, 12, 5, 3, 0, false, 2)
H3D_V(float, 3, 12, 5, 3, 0, false, 2)
H3D_V(float, 3, 12, 4, 3, 0, false, 0)
H3D_V(float, 6, 8, 4, 3, 0, false, 1)
H3D_V(float, 6, 8, 3, 3, 0, false, 2)
H3D_V(float, 6, 8, 4, 4, 0, false, 2)
H3D_V(float, 5, 8, 4, 3, 0, false, 3)
H3D_V(float, 3, 8, 5, 3, 0, false, 0)
H3D_V(float, 3, 8, 6, 3, 0, false, 0)
H3D_V(float, 4, 16, 4, 3, 0, false, 1)
H3D_V(float, 3, 16, 5, 3, 0, false, 1)
H3D_V(float, 4, 16, 4, 4, 0, false, 3)
H3D_V(float, 3, 16, 5, 6, 0, false, 3)
