// heat3d-mi355x — the tv sweep kernel's definition, included by
// stencil_tbv_impl.hpp once per wall form: H3D_TBV_NAME stencil_tbv with
// H3D_TBV_WALL 0 (no walls: the kernel as it was before the wall forms
// existed), stencil_tbv_wall with H3D_TBV_WALL 1 (insulated walls) and
// stencil_tbv_conv with H3D_TBV_WALL 2 (convective walls).  In the wall forms
// the masked step replaces the temperature of a neighbour across a wall, as the
// lean kernel's wall forms do (stencil_tbl_kernel.inc): the centre value behind
// an insulated face, the ghost fma(beta, T_inf - c, c) behind a convective one
// (an insulated face of the same call: beta = 0).  The face weights are those of
// the form without walls: Ch is read at the wall vertex.  A wave, tile or plane
// step that holds a wall-adjacent row, column or stage plane never takes the
// mask-free step, which is the code of the form without walls.
//
// H3D_TBV_CAP 1: the tc kernels (stencil_tbc*.hip), the same sweep with a heat
// capacity.  One more static field, s = dtype(1 / rc), of which a stage reads
// the centre value of the point it updates, nothing else: it is loaded where it
// is used, as the source rows are, and the update becomes kernels.hpp
// cap_update on the step's increment (steady_increment_var's chain, started
// from zero, then the source).  With H3D_TBV_CAP 0 the text is that of the tv
// kernels.
template <typename Real, int R, int WY, int K, bool SRC>
__global__ __launch_bounds__(64 * WY) void H3D_TBV_NAME(const Real* __restrict__ in, Real* __restrict__ out,
                                                       const Real* __restrict__ ch, const Real* __restrict__ src,
#if H3D_TBV_CAP
                                                       const Real* __restrict__ cap,
#endif
                                                       TBLArgs g,
#if H3D_TBV_WALL
                                                       TBLWalls wa,
#if H3D_TBV_WALL == 2
                                                       TBLConv<Real> cv,
#endif
#endif
                                                       Real Dx, Real Dy, Real Dz,
                                                       unsigned long long* res, const int* done) {
  static_assert(K >= 2 && K <= 4, "temporal depth");
  constexpr int NC = kTbvRing, PF = tbv_ahead(K);
  static_assert(NC >= K + 1 + PF, "Ch ring: planes x - K .. x + PF");
  constexpr int TY = WY * R;
  constexpr int YS = TY - 2 * K;  // tile stride along y (stored rows)
  constexpr int U = lcm_l(lcm_l(NC, 3), 2);
  static_assert(YS > 0 && R <= 16, "tile too small for depth K");
  __shared__ __attribute__((aligned(16))) Real s_row[2][K][WY][2][64];
  static_assert(sizeof(s_row) >= WY * K * sizeof(unsigned long long), "residual scratch");
  if (flag_set(done)) return;

  // piece decode (as the lean kernel: blocks dealt round-robin over the 8 XCDs)
  auto remap = [](int i, int n) {
    const int c = i & 7;
    return c * (n >> 3) + min(c, n & 7) + (i >> 3);
  };
  const int blk = blockIdx.x;
  const int zs = g.zs;
  const int ntile = g.nzb * g.nyb;
  const int nxb = g.bhi[0] - g.blo[0];
  int tt, xlo_p, xhi_p;
  {
    int pc, part;
    const int rr = g.rb & 0x3fffffff;
    if (blk < g.n1) {
      pc = remap(blk, g.n1);
      part = 0;
    } else if (blk < g.n1 + rr) {
      pc = g.n1 + remap(blk - g.n1, rr);
      part = 1;
    } else {
      pc = g.n1 + remap(blk - g.n1 - rr, rr);
      part = 2;
    }
    const int xs = pc / ntile;
    tt = pc - xs * ntile;
    const int seg = g.segsplit & 0xffff, split = g.segsplit >> 16;
    xlo_p = min(xs * seg, nxb);
    xhi_p = min(xlo_p + seg, nxb);
    if (part == 1 && (g.rb >> 30)) xhi_p = min(xhi_p, xlo_p + split);
    if (part == 2) xlo_p = min(xlo_p + split, xhi_p);
  }
  // tile order: z fastest
  const int zb = tt % g.nzb, ybk = tt / g.nzb;

  const int wave = sgpr(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int c0 = g.c00 + zb * zs;   // tile's first loaded column
  const int r0 = g.r00 + ybk * YS;  // tile's first loaded row
  const int tr0 = wave * R;         // first tile row of this wave
  const int yb = r0 + tr0;          // this wave's first row
  const int col = c0 + lane;
  const int xa = g.blo[0] + xlo_p, xe = g.blo[0] + xhi_p;
  const int x0 = xa - (K - 1), xlast = xe + K - 2;
  const int64_t sx = g.sx;

  // ---- uniform (per wave) classification
#if H3D_TBV_WALL
  // ... and holds no wall-adjacent column / row: those take the masked step
  const bool zfast = c0 >= g.uzlo && c0 + 64 <= g.uzhi && !(wa.z[0] >= c0 && wa.z[0] < c0 + 64) &&
                     !(wa.z[1] >= c0 && wa.z[1] < c0 + 64);
  const bool wrows = tr0 >= K && tr0 + R <= TY - K && yb >= g.uylo && yb + R <= g.uyhi && yb >= g.blo[1] &&
                     yb + R <= g.bhi[1] && !(wa.y[0] >= yb && wa.y[0] < yb + R) &&
                     !(wa.y[1] >= yb && wa.y[1] < yb + R);
  const bool wfast = zfast && wrows;
  // steps whose every stage is valid, updated, counted and (last stage) stored,
  // and none of whose stages' planes x - s is wall-adjacent (nothing is updated
  // below the low wall's plane or above the high wall's)
  const int xf_lo = max(max(max(x0 + 2 * (K - 1), g.ulo + K - 1), g.blo[0] + K - 1), wa.x[0] + K);
  const int xf_hi = min(min(min(xlast, g.uhi - 1), g.bhi[0] + K - 2), wa.x[1] - 1);
  // rows of this wave next to the low (bit r) / high (bit R + r) wall
  static_assert(2 * R <= 32, "wall row bits");
  unsigned wyb = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (yb + r == wa.y[0]) wyb |= 1u << r;
    if (yb + r == wa.y[1]) wyb |= 1u << (R + r);
  }
  wyb = (unsigned)sgpr((int)wyb);
#else
  const bool zfast = c0 >= g.uzlo && c0 + 64 <= g.uzhi;
  const bool wrows = tr0 >= K && tr0 + R <= TY - K && yb >= g.uylo && yb + R <= g.uyhi && yb >= g.blo[1] &&
                     yb + R <= g.bhi[1];
  const bool wfast = zfast && wrows;
  // steps whose every stage is valid, updated, counted and (last stage) stored
  const int xf_lo = max(max(x0 + 2 * (K - 1), g.ulo + K - 1), g.blo[0] + K - 1);
  const int xf_hi = min(min(xlast, g.uhi - 1), g.bhi[0] + K - 2);
#endif

  // masked form, per row r (uniform, one SGPR): bit r = row in the update
  // range, bit R + r = stored row, bit 2R + s*R + r = row counted at stage s
  static_assert(2 * R + K * R <= 32, "row mask bits");
  unsigned ybits = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = yb + r, rp = tr0 + r;
    if (row >= g.uylo && row < g.uyhi) ybits |= 1u << r;
    if (rp >= K && rp < TY - K && row >= g.blo[1] && row < g.bhi[1]) ybits |= 1u << (R + r);
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (row >= g.uylo && row < g.uyhi && rp >= s + 1 && rp < TY - s - 1 && row >= g.blo[1] - (K - 1 - s) &&
          row < g.bhi[1] + (K - 1 - s))
        ybits |= 1u << (2 * R + s * R + r);
  }
  ybits = (unsigned)sgpr((int)ybits);

  // per-lane masks (constant over the piece)
  const bool zin = col >= g.uzlo && col < g.uzhi;
  const bool zst = lane >= K && lane < K + zs && col >= g.blo[2] && col < g.bhi[2];
#if H3D_TBV_WALL
  // lanes next to the low / high z wall
  const bool zwm = col == wa.z[0], zwp = col == wa.z[1];
#endif

  // ---- addressing: uniform bases, clamped row offsets (all >= 0: clamping is
  // monotonic).  The Ch rows start one row earlier: row -1 of the wave.
  auto yclamp = [&](int row) { return min(max(row, g.ylo_live), g.yhi_live); };
  const int ybc = yclamp(yb), ybm = yclamp(yb - 1);
  const Real* __restrict__ inw = in + (g.origin + (int64_t)ybc * g.sy + c0);
  const Real* __restrict__ chw = ch + (g.origin + (int64_t)ybm * g.sy + c0);
  Real* __restrict__ outw = out + (g.origin + (int64_t)yb * g.sy + c0);
  const Real* __restrict__ srcw = SRC ? src + (g.origin + (int64_t)ybc * g.sy + c0) : nullptr;
#if H3D_TBV_CAP
  // the capacity field has the field's layout (StencilParams::cap: L.bytes()),
  // and it is read at T's own clamped plane, row and lane offsets: every offset
  // that is in bounds for T is in bounds for s
  const Real* __restrict__ capw = cap + (g.origin + (int64_t)ybc * g.sy + c0);
#endif
  int roff[R], coff[R + 2];
#pragma unroll
  for (int r = 0; r < R; ++r) roff[r] = sgpr((yclamp(yb + r) - ybc) * (int)g.sy * (int)sizeof(Real));
#pragma unroll
  for (int r = 0; r < R + 2; ++r) coff[r] = sgpr((yclamp(yb - 1 + r) - ybm) * (int)g.sy * (int)sizeof(Real));
  const int sy_b = (int)g.sy * (int)sizeof(Real);
  const unsigned lane_b = (unsigned)lane * (unsigned)sizeof(Real);

  Real q[3][R];          // T^n ring: plane p in slot (p - x0 + 1) mod 3
  Real f[K - 1][3][R];   // F_{s+1}(p) in f[s][(p + s) mod 3]
  Real h[NC][R + 2];     // Ch ring: plane p in slot (p - x0 + K) mod NC; row r of the wave in h[.][r + 1]
  Real m[K];             // per-lane residual maxima (field precision, widened at the end)
  bool nan_seen = false;
#pragma unroll
  for (int s = 0; s < K; ++s) m[s] = Real(0);
#pragma unroll
  for (int s = 0; s < K - 1; ++s)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int r = 0; r < R; ++r) f[s][i][r] = Real(0);

  auto xclamp = [&](int x) { return min(max(x, g.xlo_live), g.xhi_live); };
  auto load_plane = [&](int x, Real (&d)[R]) {
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(inw + (int64_t)xclamp(x) * sx);
#pragma unroll
    for (int r = 0; r < R; ++r) d[r] = buf_load<Real>(rs, lane_b, roff[r]);
  };
  auto load_ch = [&](int x, Real (&d)[R + 2]) {
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(chw + (int64_t)xclamp(x) * sx);
#pragma unroll
    for (int r = 0; r < R + 2; ++r) d[r] = buf_load<Real>(rs, lane_b, coff[r]);
  };
  // before step x0: T^n planes x0 - 1 .. x0 + 1, Ch planes x0 - K .. x0 + PF - 1
#pragma unroll
  for (int i = 0; i < 3; ++i) load_plane(x0 - 1 + i, q[i]);
#pragma unroll
  for (int i = 0; i < K + PF; ++i) load_ch(x0 - K + i, h[i]);

  // One plane step.  FAST: every condition below is known true.
  auto step = [&](auto fast_tag, const int x, auto ph_tag) {
    constexpr bool FAST = decltype(fast_tag)::value;
    constexpr int ph = decltype(ph_tag)::value;
    constexpr int sM = ph % 3, sC = (ph + 1) % 3, sP = (ph + 2) % 3;
    constexpr int fw = ph % 3, fc = (ph + 2) % 3, fm = (ph + 1) % 3;
    constexpr int par = ph & 1;  // LDS buffer (U is even)
    // Ch plane x + PF into the slot of plane x + PF - NC <= x - K - 1, which no stage reads any more
    load_ch(x + PF, h[(ph + K + PF) % NC]);
    // publish the edge rows of every stage's centre plane
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const Real(&C)[R] = s == 0 ? q[sC] : f[s > 0 ? s - 1 : 0][fc];
      s_row[par][s][wave][0][lane] = C[0];
      s_row[par][s][wave][1][lane] = C[R - 1];
    }
    __syncthreads();
    const int wl = max(wave - 1, 0), wh = min(wave + 1, WY - 1);
#pragma unroll
    for (int s = 0; s < K; ++s) {
      Real(&M)[R] = s == 0 ? q[sM] : f[s > 0 ? s - 1 : 0][fm];
      Real(&C)[R] = s == 0 ? q[sC] : f[s > 0 ? s - 1 : 0][fc];
      Real(&P)[R] = s == 0 ? q[sP] : f[s > 0 ? s - 1 : 0][fw];
      const Real lo = s_row[par][s][wl][1][lane];
      const Real hi = s_row[par][s][wh][0][lane];
      const int p = x - s;
      // Ch of planes p - 1, p, p + 1 (plane x sits in slot (ph + K) mod NC)
      const Real(&HM)[R + 2] = h[(ph + K - s - 1 + NC) % NC];
      const Real(&HC)[R + 2] = h[(ph + K - s) % NC];
      const Real(&HP)[R + 2] = h[(ph + K - s + 1) % NC];
      Real S[R];
      if constexpr (SRC) {
        const __amdgpu_buffer_rsrc_t rs = plane_rsrc(srcw + (int64_t)xclamp(p) * sx);
#pragma unroll
        for (int r = 0; r < R; ++r) S[r] = buf_load<Real>(rs, lane_b, roff[r]);
      }
#if H3D_TBV_CAP
      // s on this stage's plane, the wave's own rows, the lane's own column (it
      // has no neighbours: no ring).  A clamped plane or row only ever feeds a
      // masked-out result, as T's, Ch's and S's do.
      Real A[R];
      {
        const __amdgpu_buffer_rsrc_t rs = plane_rsrc(capw + (int64_t)xclamp(p) * sx);
#pragma unroll
        for (int r = 0; r < R; ++r) A[r] = buf_load<Real>(rs, lane_b, roff[r]);
      }
#endif
      // masked form: uniform x conditions of this stage
      bool xin = true, xcnt = true, xst = true;
      if constexpr (!FAST) {
        xin = p >= g.ulo && p < g.uhi;
        xcnt = xin && x >= x0 + 2 * s && x <= xlast && p >= g.blo[0] - (K - 1 - s) && p < g.bhi[0] + (K - 1 - s);
        xst = p >= xa && p < xe;
      }
#if H3D_TBV_WALL
      // this stage's plane is next to the low / high wall of the marching axis
      const bool wxm = !FAST && p == wa.x[0], wxp = !FAST && p == wa.x[1];
#endif
#pragma unroll
      for (int r = 0; r < R; ++r) {
#if H3D_TBV_WALL
        Real ym = r == 0 ? lo : C[r > 0 ? r - 1 : 0];
        Real yp = r == R - 1 ? hi : C[r + 1 < R ? r + 1 : 0];
        Real zm = dpp_shr1z(C[r]);
        Real zp = dpp_shl1z(C[r]);
        Real xm = M[r], xp = P[r];
        if constexpr (!FAST) {
#if H3D_TBV_WALL == 2
          // the convective ghost of each face (kernels.hpp convective_ghost; beta
          // 0: the mirror ghost of an insulated wall)
          const Real da = cv.tinf - C[r];
          if (wxm) xm = h3d_fma(cv.x[0], da, C[r]);
          if (wxp) xp = h3d_fma(cv.x[1], da, C[r]);
          if ((wyb >> r) & 1) ym = h3d_fma(cv.y[0], da, C[r]);
          if ((wyb >> (R + r)) & 1) yp = h3d_fma(cv.y[1], da, C[r]);
          zm = zwm ? h3d_fma(cv.z[0], da, C[r]) : zm;
          zp = zwp ? h3d_fma(cv.z[1], da, C[r]) : zp;
#else
          // the mirror ghost: the neighbour across an insulated wall is the centre value
          if (wxm) xm = C[r];
          if (wxp) xp = C[r];
          if ((wyb >> r) & 1) ym = C[r];
          if ((wyb >> (R + r)) & 1) yp = C[r];
          zm = zwm ? C[r] : zm;
          zp = zwp ? C[r] : zp;
#endif
        }
#else
        const Real ym = r == 0 ? lo : C[r > 0 ? r - 1 : 0];
        const Real yp = r == R - 1 ? hi : C[r + 1 < R ? r + 1 : 0];
        const Real zm = dpp_shr1z(C[r]);
        const Real zp = dpp_shl1z(C[r]);
        const Real xm = M[r], xp = P[r];
#endif
        const Real hc = HC[r + 1];
        // the six face weights, each the one rounded add of ftcs_update_var
        const Real wxm = hc + HM[r + 1], wxp = hc + HP[r + 1];
        const Real wym = hc + HC[r], wyp = hc + HC[r + 2];
        const Real wzm = hc + dpp_shr1z(hc), wzp = hc + dpp_shl1z(hc);
#if H3D_TBV_CAP
        // the increment of the step, then the source, then T' = fma(s, u, T)
        Real u = steady_increment_varw<Real>(C[r], xm, xp, ym, yp, zm, zp, wxm, wxp, wym, wyp, wzm, wzp, Dx, Dy, Dz);
        if constexpr (SRC) u = add_source<Real>(u, S[r]);
        const Real nv = cap_update<Real>(A[r], u, C[r]);
#else
        Real nv = ftcs_update_varw<Real>(C[r], xm, xp, ym, yp, zm, zp, wxm, wxp, wym, wyp, wzm, wzp, Dx, Dy, Dz);
        if constexpr (SRC) nv = add_source<Real>(nv, S[r]);
#endif
        const Real d = resid_abs_r(nv, C[r]);
        bool upd = true, cnt = true, st = true;
        if constexpr (!FAST) {
          upd = xin && ((ybits >> r) & 1);
          cnt = xcnt && ((ybits >> (2 * R + s * R + r)) & 1);
          st = xst && ((ybits >> (R + r)) & 1);
        }
        if (s < K - 1) {
          Real(&N)[R] = f[s < K - 1 ? s : 0][fw];
          if constexpr (FAST) N[r] = nv;
          else N[r] = (upd && zin) ? nv : C[r];
        }
        if constexpr (FAST) {
          m[s] = fmax(m[s], d);
        } else {
          if (cnt) m[s] = fmax(m[s], d);
        }
        if (s == K - 1 && st) {
          // T^{n+K} on the stored region (inside the box, hence the update range)
          nan_seen |= zst && (nv != nv);
          if (zst) buf_store<Real, 0>(nv, plane_rsrc(outw + (int64_t)p * sx), lane_b, r * sy_b);
        }
      }
      // the slot stage 0 has just freed
      if (s == 0) load_plane(x + 2, q[sM]);
    }
  };

  // whole chunks of U steps (the unrolled body needs a constant trip count);
  // padded steps past xlast take the masked form and count / store nothing
  if (xa < xe) {
    for (int xb = x0; xb <= xlast; xb += U) {
      static_for<0, U>([&](auto ph_tag) {
        constexpr int ph = decltype(ph_tag)::value;
        const int x = xb + ph;
        if (wfast && x >= xf_lo && x <= xf_hi) step(std::true_type{}, x, ph_tag);
        else step(std::false_type{}, x, ph_tag);
      });
    }
  }

  // this piece's residuals (the lane masks depend on its tile)
  if (res) {
    double mm[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      // stage s counts lanes inside its cone, the update range and the box
      // widened by K-1-s (deep-halo points still in flight stay excluded)
      const bool ok = zin && lane >= s + 1 && lane < 63 - s && col >= g.blo[2] - (K - 1 - s) &&
                      col < g.bhi[2] + (K - 1 - s);
      mm[s] = ok ? (double)m[s] : 0.0;
    }
    // the row exchange buffer is dead: reuse it for the per-wave maxima
    __syncthreads();
    residual_commit_block<WY, K>(res, mm, nan_seen,
                                 *reinterpret_cast<unsigned long long(*)[WY][K]>(&s_row[0][0][0][0][0]));
  }
}
