// Heat-source forms of the lean sweep kernel (stencil_tbl_impl.hpp stencil_tbl_src,
// launch_tbl<..., SRC = true>): H3D_VS(Real, R, WY, K, Q, NTS, SW, PART), as
// stencil_tbl_variants.inc.  Exactly the variants a solver with a source picks by
// default at the default depth 3: the K = 3 sweep, the long K = 4 sweep and the
// partial K = 2 sweep, fp64 with every residual and with the last one only (fp32
// source runs compute every residual), and the y-marching thin-slab forms.
// The dispatch is this list (stencil_tbl.hip hands it, as types, to
// stencil_tbl_form.hpp dispatch_tbl_form); any other spec with a source is an
// error.  There is no edge role with a source.
H3D_VS(double, 2, 5, 3, 3, 2, true, 0)
H3D_VS(double, 3, 3, 3, 3, 2, true, 1)
H3D_VS(double, 3, 4, 4, 3, 2, true, 3)
H3D_VS(double, 3, 16, 3, 3, 2, false, 2)
H3D_VS(double, 3, 16, 3, 3, 66, false, 3)
H3D_VS(double, 3, 12, 4, 3, 2, false, 1)
H3D_VS(double, 3, 12, 4, 3, 66, false, 2)
H3D_VS(double, 5, 16, 2, 3, 2, false, 0)
H3D_VS(double, 5, 16, 2, 3, 66, false, 1)
H3D_VS(float, 2, 5, 3, 3, 0, true, 2)
H3D_VS(float, 3, 3, 3, 3, 0, true, 0)
H3D_VS(float, 3, 4, 4, 3, 0, true, 2)
H3D_VS(float, 3, 16, 3, 3, 0, false, 1)
H3D_VS(float, 4, 16, 4, 3, 0, false, 3)
H3D_VS(float, 3, 16, 2, 3, 0, false, 0)
