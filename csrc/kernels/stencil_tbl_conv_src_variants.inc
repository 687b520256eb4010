// Convective-wall forms of the lean sweep kernel with a heat source (stencil_tbl_impl.hpp
// stencil_tbl_conv_src, launch_tbl<..., SRC = true, 0, WALL = 2>): H3D_VCS(Real, R, WY, K,
// Q, NTS, SW), the fields of stencil_tbl_conv_variants.inc, all instantiated in
// stencil_tbl_conv_src.hip.  The list mirrors stencil_tbl_src_variants.inc: the K = 3
// sweep, the long K = 4 sweep and the partial K = 2 sweep for both dtypes, fp64 also
// with the last residual only, and the y-marching thin-slab forms of x-slab boundary
// pieces.  dispatch_tbl_conv_src names every entry; any other spec with a convective
// face and a source is an error.  No entry uses scratch (profiles/wall_source_sweeps.md):
// where the source list's shape would (fp64 3 x 16 at K = 3 and 3 x 12 at K = 4 with every
// residual, 5 x 16 at K = 2 in both residual forms, fp32 4 x 16 at K = 4) the entry is a
// shape of 12 or 8 waves, to which the dispatch also sends the default spec.
H3D_VCS(double, 2, 5, 3, 3, 2, true)
H3D_VCS(double, 3, 3, 3, 3, 2, true)
H3D_VCS(double, 3, 4, 4, 3, 2, true)
H3D_VCS(double, 4, 12, 3, 3, 2, false)
H3D_VCS(double, 3, 16, 3, 3, 66, false)
H3D_VCS(double, 5, 8, 4, 3, 2, false)
H3D_VCS(double, 3, 12, 4, 3, 66, false)
H3D_VCS(double, 6, 12, 2, 3, 2, false)
H3D_VCS(double, 6, 12, 2, 3, 66, false)
H3D_VCS(float, 2, 5, 3, 3, 0, true)
H3D_VCS(float, 3, 3, 3, 3, 0, true)
H3D_VCS(float, 3, 4, 4, 3, 0, true)
H3D_VCS(float, 3, 16, 3, 3, 0, false)
H3D_VCS(float, 4, 12, 4, 3, 0, false)
H3D_VCS(float, 3, 16, 2, 3, 0, false)
