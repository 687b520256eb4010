// Convective-wall forms of the lean sweep kernel (stencil_tbl_impl.hpp stencil_tbl_conv,
// launch_tbl<..., WALL = 2>): H3D_VC(Real, R, WY, K, Q, NTS, SW), the fields of
// stencil_tbl_wall_variants.inc, all instantiated in stencil_tbl_conv.hip.  The list
// mirrors the insulated-wall one: the default shapes at depth 2, 3 and 4 for both
// dtypes, fp64 also with the last residual only, and the y-marching thin-slab forms
// of x-slab boundary pieces.  dispatch_tbl_conv names every entry; any other spec
// with a convective face is an error.
H3D_VC(double, 2, 5, 3, 3, 2, true)
H3D_VC(double, 3, 3, 3, 3, 2, true)
H3D_VC(double, 3, 4, 4, 3, 2, true)
H3D_VC(double, 3, 16, 3, 3, 2, false)
H3D_VC(double, 3, 16, 3, 3, 66, false)
H3D_VC(double, 3, 12, 4, 3, 2, false)
H3D_VC(double, 3, 12, 4, 3, 66, false)
H3D_VC(double, 5, 16, 2, 3, 2, false)
H3D_VC(double, 5, 16, 2, 3, 66, false)
H3D_VC(float, 2, 5, 3, 3, 0, true)
H3D_VC(float, 3, 3, 3, 3, 0, true)
H3D_VC(float, 3, 4, 4, 3, 0, true)
H3D_VC(float, 3, 16, 3, 3, 0, false)
H3D_VC(float, 4, 16, 4, 3, 0, false)
H3D_VC(float, 3, 16, 2, 3, 0, false)
