// Insulated-wall forms of the lean sweep kernel (stencil_tbl_impl.hpp stencil_tbl_wall,
// launch_tbl<..., WALL = true>): H3D_VW(Real, R, WY, K, Q, NTS, SW), the fields of
// stencil_tbl_variants.inc without the instantiation unit (all are instantiated in
// stencil_tbl_wall.hip).  Exactly the variants a solver with insulated walls picks
// by default at the default depth 3: the K = 3 sweep, the partial K = 2 sweep and
// the long K = 4 sweep, one value per lane, fp64 with every residual and with the
// last one only (fp32 wall runs compute every residual), and the y-marching
// thin-slab forms of x-slab boundary pieces.  dispatch_tbl_wall names every entry;
// any other spec with walls is an error.
H3D_VW(double, 2, 5, 3, 3, 2, true)
H3D_VW(double, 3, 3, 3, 3, 2, true)
H3D_VW(double, 3, 4, 4, 3, 2, true)
H3D_VW(double, 3, 16, 3, 3, 2, false)
H3D_VW(double, 3, 16, 3, 3, 66, false)
H3D_VW(double, 3, 12, 4, 3, 2, false)
H3D_VW(double, 3, 12, 4, 3, 66, false)
H3D_VW(double, 5, 16, 2, 3, 2, false)
H3D_VW(double, 5, 16, 2, 3, 66, false)
H3D_VW(float, 2, 5, 3, 3, 0, true)
H3D_VW(float, 3, 3, 3, 3, 0, true)
H3D_VW(float, 3, 4, 4, 3, 0, true)
H3D_VW(float, 3, 16, 3, 3, 0, false)
H3D_VW(float, 4, 16, 4, 3, 0, false)
H3D_VW(float, 3, 16, 2, 3, 0, false)
