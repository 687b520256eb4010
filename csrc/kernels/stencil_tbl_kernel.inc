// heat3d-mi355x — the lean K-step sweep kernel's definition, included by
// stencil_tbl_impl.hpp once per form: H3D_TBL_NAME stencil_tbl with
// H3D_TBL_SRC 0, and stencil_tbl_src with H3D_TBL_SRC 1 (heat source, see the
// comment there).  Textual inclusion keeps the kernel without a source exactly
// the code it was before the source form existed.  H3D_TBL_WALL 1 (kernel
// stencil_tbl_wall, stencil_tbl_wall.hip) is the insulated-wall form: in the
// masked step a neighbour across an insulated wall is replaced by the centre
// value (impl.hpp), and a wave or plane step that holds a wall-adjacent row,
// column or plane never takes the mask-free step.  H3D_TBL_WALL 2 (kernel
// stencil_tbl_conv, stencil_tbl_conv.hip) is the convective-wall form: the same
// masked step, with the ghost fma(beta, T_inf - c, c) of the face (TBLConv) in
// place of the centre value c; an insulated face enters with beta = 0.
// H3D_TBL_SRC 1 together with H3D_TBL_WALL 1 / 2 (kernels stencil_tbl_wall_src /
// stencil_tbl_conv_src, stencil_tbl_wall_src.hip / stencil_tbl_conv_src.hip): the
// wall step with the source rows of the source form; the ghost substitution
// comes first, the source is added to the finished update.
//
// EW > 0: the edge role (impl.hpp, third step form).  Waves 0 and WY - 1 hold
// the tile's K halo rows and E = EW - 1 owned rows next to them (R + E rows; the
// tile has WY * R + 2E rows) and evaluate, for each row, only the stages whose
// output lies inside the tile's cone.  EW = 0 is the kernel without the role.
template <typename Real, int R, int WY, int K, int Q, int NTS = 0, bool SW = false, int EW = 0>
__global__ __launch_bounds__(64 * WY) void H3D_TBL_NAME(const Real* __restrict__ in, Real* __restrict__ out,
#if H3D_TBL_SRC
                                                       const Real* __restrict__ src,
#endif
                                                       TBLArgs g,
#if H3D_TBL_WALL
                                                       TBLWalls wa,
#if H3D_TBL_WALL == 2
                                                       TBLConv<Real> cv,
#endif
#endif
                                                       Real Dx, Real Dy, Real Dz,
                                                       unsigned long long* res, const int* done) {
  static_assert(K >= 2 && K <= 6, "temporal depth");
  // T^n ring: Q = 3 loads plane x+2 into the slot stage 0 frees at step x
  // ((K-1)/K of a step of latency cover); Q >= 4 loads plane x+Q-2 at the
  // start of step x (Q-3 steps of cover)
  static_assert(Q == 3 || Q == 4 || Q == 6, "T^n ring size");
  constexpr bool EDGE = EW > 0;
  constexpr int E = EDGE ? EW - 1 : 0;  // owned rows of an edge wave
  constexpr int RB = R + E;             // rows of an edge wave (register rows of every wave)
  static_assert(!EDGE || (R >= K && WY >= 3 && !SW && !H3D_TBL_SRC), "edge role: halo-only waves, no source form");
#if H3D_TBL_WALL
  static_assert(!EDGE, "the wall form has no edge role");
#endif
  constexpr int TY = WY * R + 2 * E;
  constexpr int YS = TY - 2 * K;   // tile stride along y (stored rows)
  // x-loop unroll making every ring index and the LDS parity static
  constexpr int U = lcm_l(lcm_l(Q, 3), 2);
  static_assert(YS > 0 && R <= 16, "tile too small for depth K");
  // NTS bit kResidualLastOnly: only the last step's residual (monotone check)
  constexpr bool RL = (NTS & kResidualLastOnly) != 0;
  constexpr int ST = NTS & ~kResidualLastOnly;  // the stores' cache-policy bits
  __shared__ __attribute__((aligned(16))) Real s_row[2][K][WY][2][64];
  static_assert(sizeof(s_row) >= WY * K * sizeof(unsigned long long), "residual scratch");
  if (flag_set(done)) {
    if (g.fst) fused_check_tail<K, RL>(g.fst, g.fslot, g.fblocks);
    return;
  }

  // piece decode: blocks dealt round-robin over the 8 XCDs; consecutive
  // pieces (neighbouring tiles) share an XCD's L2 (same encoding as tbr)
  auto remap = [](int i, int n) {
    const int c = i & 7;
    return c * (n >> 3) + min(c, n & 7) + (i >> 3);
  };
  const int blk = blockIdx.x;
  const int zs = g.zs;
  const int ntile = g.nzb * g.nyb;
  const int nxb = g.bhi[0] - g.blo[0];
  // This workgroup's piece: plane steps [w, wend) of the tile-major list
  // (tile t, plane x) -> t * nxb + x, one piece per block, x segments of
  // `seg` planes (plan_x: whole rounds of pieces, then a split tail); each
  // piece pays the 2(K-1)-plane pipeline fill.  (The persistent walk of round 3,
  // every block a contiguous 1/n of the list, measured 18-22% slower on
  // MI355X: the x plan's concurrent workgroups sweep neighbouring tiles over
  // the same x planes, so their overlapping halo rows are L2 hits.)
  int64_t w, wend;
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
    const int tt = pc - xs * ntile;
    const int seg = g.segsplit & 0xffff, split = g.segsplit >> 16;
    int xlo_p = xs * seg, xhi_p = min(xlo_p + seg, nxb);
    if (part == 1 && (g.rb >> 30)) xhi_p = min(xhi_p, xlo_p + split);
    if (part == 2) xlo_p = min(xlo_p + split, xhi_p);
    w = (int64_t)tt * nxb + xlo_p;
    wend = (int64_t)tt * nxb + xhi_p;
  }

  // tile order: z fastest
  const int tt = (int)(w / nxb);
  const int xlo_p = (int)(w - (int64_t)tt * nxb);
  const int xhi_p = (int)min((int64_t)nxb, xlo_p + (wend - w));
  const int zb = tt % g.nzb, ybk = tt / g.nzb;

  const int wave = sgpr(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int c0 = g.c00 + zb * zs;         // tile's first loaded column
  const int r0 = g.r00 + ybk * YS;          // tile's first loaded row
  // first tile row of this wave (edge role: wave 0 holds R + E rows)
  const int tr0 = EDGE && wave > 0 ? E + wave * R : wave * R;
  const int yb = r0 + tr0;                  // this wave's first row
  const int col = c0 + lane;
  const int xa = g.blo[0] + xlo_p, xe = g.blo[0] + xhi_p;
  const int x0 = xa - (K - 1), xlast = xe + K - 2;
  const int64_t sx = g.sx;

  // ---- uniform (per wave) classification
#if H3D_TBL_WALL
  // ... and holds no wall-adjacent column / row: those take the masked step
  const bool zfast = c0 >= g.uzlo && c0 + 64 <= g.uzhi && !(wa.z[0] >= c0 && wa.z[0] < c0 + 64) &&
                     !(wa.z[1] >= c0 && wa.z[1] < c0 + 64);
  const bool wrows = tr0 >= K && tr0 + R <= TY - K && yb >= g.uylo && yb + R <= g.uyhi &&
                     yb >= g.blo[1] && yb + R <= g.bhi[1] && !(wa.y[0] >= yb && wa.y[0] < yb + R) &&
                     !(wa.y[1] >= yb && wa.y[1] < yb + R);
  const bool wfast = zfast && wrows;
  // steps whose every stage is valid, updated, counted and (last stage) stored,
  // and none of whose stages' planes x - s is wall-adjacent (nothing is updated
  // below the low wall's plane or above the high wall's)
  const int xf_lo = max(max(max(x0 + 2 * (K - 1), g.ulo + K - 1), g.blo[0] + K - 1), wa.x[0] + K);
  const int xf_hi = min(min(min(xlast, g.uhi - 1), g.bhi[0] + K - 2), wa.x[1] - 1);
  // rows of this wave next to the low (bit r) / high (bit RB + r) wall
  static_assert(2 * RB <= 32, "wall row bits");
  unsigned wyb = 0;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (yb + r == wa.y[0]) wyb |= 1u << r;
    if (yb + r == wa.y[1]) wyb |= 1u << (RB + r);
  }
  wyb = (unsigned)sgpr((int)wyb);
#else
  const bool zfast = c0 >= g.uzlo && c0 + 64 <= g.uzhi;
  const bool wrows = tr0 >= K && tr0 + R <= TY - K && yb >= g.uylo && yb + R <= g.uyhi &&
                     yb >= g.blo[1] && yb + R <= g.bhi[1];
  const bool wfast = zfast && wrows;
  // steps whose every stage is valid, updated, counted and (last stage) stored
  const int xf_lo = max(max(x0 + 2 * (K - 1), g.ulo + K - 1), g.blo[0] + K - 1);
  const int xf_hi = min(min(xlast, g.uhi - 1), g.bhi[0] + K - 2);
#endif

  // masked form, per row r (uniform, one SGPR): bit r = row in the update
  // range, bit R + r = stored row, bit 2R + s*R + r = row counted at stage s
  // (64-bit when the rows x stages outgrow one SGPR: 8-wave tiles of 6 rows)
  // (edge role: RB rows per field, as an edge wave holds)
  using YMask = std::conditional_t<(2 * RB + K * RB <= 32), unsigned, unsigned long long>;
  static_assert(2 * RB + K * RB <= 64, "row mask bits");
  YMask ybits = 0;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const int row = yb + r, rp = tr0 + r;
    if (row >= g.uylo && row < g.uyhi) ybits |= YMask(1) << r;
    if (rp >= K && rp < TY - K && row >= g.blo[1] && row < g.bhi[1]) ybits |= YMask(1) << (RB + r);
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (row >= g.uylo && row < g.uyhi && rp >= s + 1 && rp < TY - s - 1 && row >= g.blo[1] - (K - 1 - s) &&
          row < g.bhi[1] + (K - 1 - s))
        ybits |= YMask(1) << (2 * RB + s * RB + r);
  }
  if constexpr (sizeof(YMask) == 4) {
    ybits = (unsigned)sgpr((int)ybits);
  } else {
    ybits = ((YMask)(unsigned)sgpr((int)(ybits >> 32)) << 32) | (unsigned)sgpr((int)(unsigned)ybits);
  }

  // per-lane masks (constant over the piece)
  const bool zin = col >= g.uzlo && col < g.uzhi;
  const bool zst = lane >= K && lane < K + zs && col >= g.blo[2] && col < g.bhi[2];
#if H3D_TBL_WALL
  // lanes next to the low / high z wall
  const bool zwm = col == wa.z[0], zwp = col == wa.z[1];
#endif

  // ---- addressing: uniform base of row yb, column c0; clamped row offsets
  // (uniform by construction: kernel arguments and the readfirstlane'd wave
  // index; pointers stay in the global address space)
  // Loads: base at the wave's first clamped row; a buffer soffset is an
  // unsigned 32-bit value, so every row offset must be >= 0 (clamping is
  // monotonic: clamp(yb + r) >= clamp(yb)).  Stores only touch stored rows,
  // which are real rows at or after yb.
  auto yclamp = [&](int row) { return min(max(row, g.ylo_live), g.yhi_live); };
  const int ybc = yclamp(yb);
  const Real* __restrict__ inw = in + (g.origin + (int64_t)ybc * g.sy + c0);
  Real* __restrict__ outw = out + (g.origin + (int64_t)yb * g.sy + c0);
#if H3D_TBL_SRC
  const Real* __restrict__ srcw = src + (g.origin + (int64_t)ybc * g.sy + c0);
#endif
  // row byte offsets (clamped rows fold in), 0 <= roff < 2^31: checked in launch_tbl
  int roff[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) roff[r] = sgpr((yclamp(yb + r) - ybc) * (int)g.sy * (int)sizeof(Real));
  const int sy_b = (int)g.sy * (int)sizeof(Real);
  const unsigned lane_b = (unsigned)lane * (unsigned)sizeof(Real);

  Real q[Q][RB];             // T^n ring: plane p in slot (p - x0 + 1) mod Q
  Real f[K - 1][3][RB];      // F_{s+1}(p) in f[s][(p + s) mod 3]
  Real m[K];                 // per-lane residual maxima (field precision, widened at the end)
  bool nan_seen = false;
#pragma unroll
  for (int s = 0; s < K; ++s) m[s] = Real(0);
  if constexpr (!EDGE) {
#pragma unroll
    for (int s = 0; s < K - 1; ++s)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) f[s][i][r] = Real(0);
  }

  // rows [B, N) of plane x
  auto load_rows = [&](int x, Real (&d)[RB], auto b_tag, auto n_tag) {
    const int xc = min(max(x, g.xlo_live), g.xhi_live);
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(inw + (int64_t)xc * sx);
#pragma unroll
    for (int r = decltype(b_tag)::value; r < decltype(n_tag)::value; ++r) d[r] = buf_load<Real>(rs, lane_b, roff[r]);
  };
  auto load_plane = [&](int x, Real (&d)[RB]) {
    const int xc = min(max(x, g.xlo_live), g.xhi_live);
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(inw + (int64_t)xc * sx);
#pragma unroll
    for (int r = 0; r < R; ++r) d[r] = buf_load<Real>(rs, lane_b, roff[r]);
  };
  constexpr int NPRE = Q == 3 ? 3 : Q - 1;  // planes resident / in flight before step x0
  if constexpr (!EDGE) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) load_plane(x0 - 1 + i, q[i]);
  }

  // One plane step.  FORM (impl.hpp StepForm): kStepFree, every condition below
  // is known true; kStepZ (edge-role kernels only), the x and y conditions are
  // known true and the lanes outside the z update range pass their centre value
  // on; kStepMasked, every condition is evaluated.  ROLE: 0 an
  // interior wave (R rows, every stage); 1 / 2 the edge role of wave 0 /
  // WY - 1: RB rows, and of row r only the stages inside the tile's cone
  // (static, so the stage rings outside it are never allocated).  The stage-s
  // output of tile row rp is read only by stage s + 1 of rows rp - 1 .. rp + 1,
  // and stage s is valid on rows [s + 1, TY - s - 1): everything a cone value
  // reads is in the cone, whatever the masks say.
  auto step = [&](auto form_tag, const int x, auto ph_tag, auto role_tag) {
    constexpr int FORM = decltype(form_tag)::value;
    constexpr bool FAST = FORM != kStepMasked;  // no x / y condition is evaluated
    constexpr bool ZSEL = FORM == kStepZ;
    static_assert(!ZSEL || EDGE, "the z-masked step exists in the edge-role kernels only");
    constexpr int ph = decltype(ph_tag)::value;
    constexpr int ROLE = decltype(role_tag)::value;
    constexpr int NR = ROLE ? RB : R;
    // is stage s of local row r inside the cone?
    auto live = [](int r, int s) constexpr { return ROLE == 0 || (ROLE == 1 ? s < r : s < RB - 1 - r); };
    constexpr int sM = ph % Q, sC = (ph + 1) % Q, sP = (ph + 2) % Q;
    constexpr int fw = ph % 3, fc = (ph + 2) % 3, fm = (ph + 1) % 3;
    constexpr int par = ph & 1;  // LDS buffer (U is even)
    if constexpr (Q >= 4) {
      if constexpr (!EDGE) load_plane(x + Q - 2, q[(ph + Q - 1) % Q]);
      else load_rows(x + Q - 2, q[(ph + Q - 1) % Q], std::integral_constant<int, 0>{}, std::integral_constant<int, NR>{});
    }
    // publish the edge rows of every stage's centre plane
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const Real(&C)[RB] = s == 0 ? q[sC] : f[s > 0 ? s - 1 : 0][fc];
      // (an edge wave publishes the row its one neighbour reads)
      if constexpr (ROLE != 1) s_row[par][s][wave][0][lane] = C[0];
      if constexpr (ROLE != 2) s_row[par][s][wave][1][lane] = C[NR - 1];
    }
    __syncthreads();
    const int wl = max(wave - 1, 0), wh = min(wave + 1, WY - 1);
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if constexpr (EDGE && !FAST) {
        // Dead stage of the pipeline fill (uniform: one scalar branch).  The
        // piece stores planes [xa, xe) at stage K - 1, and the stage-s output of
        // plane p is read only by stage s + 1 of planes p - 1 .. p + 1, so the
        // piece needs stage s on the planes p >= xa - (K - 1 - s) = x0 + s only
        // (the cone along x).  Stage s meets plane p at step p + s: before step
        // x0 + 2s its plane is below that cone.  Such a stage counts and stores
        // nothing (xcnt asks for x >= x0 + 2s; the first stored plane xa meets
        // stage K - 1 at step x0 + 2(K - 1)), and what it would write, stage
        // s + 1's input on a plane below x0 + s, is read by no needed stage:
        // stage s + 1 is needed from step x0 + 2s + 2 on, where its plane is
        // x0 + s + 1 or above and its lowest input plane x0 + s.  Everything a
        // cone value reads is in the cone, so the stage's rows are skipped and
        // its ring slot keeps whatever it held; the stages that would read that
        // are dead themselves.  Stage 0 is never dead, so the ring load below
        // it is not skipped; the rows published above and the barrier are those
        // of every step.  (The other end has no dead stage: every stage meets
        // the last plane it needs, xe - 1 + (K - 1 - s), at step xlast; the
        // padded steps after xlast are left by the caller.)
        if (s > 0 && x < x0 + 2 * s) continue;
      }
      Real(&M)[RB] = s == 0 ? q[sM] : f[s > 0 ? s - 1 : 0][fm];
      Real(&C)[RB] = s == 0 ? q[sC] : f[s > 0 ? s - 1 : 0][fc];
      Real(&P)[RB] = s == 0 ? q[sP] : f[s > 0 ? s - 1 : 0][fw];
      const Real lo = s_row[par][s][wl][1][lane];
      const Real hi = s_row[par][s][wh][0][lane];
      const int p = x - s;
#if H3D_TBL_SRC
      // the source rows of this stage's plane (clamped as load_plane)
      Real S[RB];
      {
        const int pc = min(max(p, g.xlo_live), g.xhi_live);
        const __amdgpu_buffer_rsrc_t rs = plane_rsrc(srcw + (int64_t)pc * sx);
#pragma unroll
        for (int r = 0; r < R; ++r) S[r] = buf_load<Real>(rs, lane_b, roff[r]);
      }
#endif
      // masked form: uniform x conditions of this stage
      bool xin = true, xcnt = true, xst = true;
      if constexpr (!FAST) {
        xin = p >= g.ulo && p < g.uhi;
        xcnt = xin && x >= x0 + 2 * s && x <= xlast && p >= g.blo[0] - (K - 1 - s) && p < g.bhi[0] + (K - 1 - s);
        xst = p >= xa && p < xe;
      }
#if H3D_TBL_WALL
      // this stage's plane is next to the low / high wall of the marching axis
      const bool wxm = !FAST && p == wa.x[0], wxp = !FAST && p == wa.x[1];
#endif
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (!live(r, s)) continue;
#if H3D_TBL_WALL
        Real ym = r == 0 ? lo : C[r > 0 ? r - 1 : 0];
        Real yp = r == NR - 1 ? hi : C[r + 1 < NR ? r + 1 : 0];
        Real zm = dpp_shr1z(C[r]);
        Real zp = dpp_shl1z(C[r]);
        Real xm = M[r], xp = P[r];
#if H3D_TBL_WALL == 2
        if constexpr (!FAST) {
          // the convective ghost of each face (kernels.hpp convective_ghost; beta
          // 0: the mirror ghost of an insulated wall)
          const Real da = cv.tinf - C[r];
          if (wxm) xm = h3d_fma(cv.x[0], da, C[r]);
          if (wxp) xp = h3d_fma(cv.x[1], da, C[r]);
          if ((wyb >> r) & 1) ym = h3d_fma(cv.y[0], da, C[r]);
          if ((wyb >> (RB + r)) & 1) yp = h3d_fma(cv.y[1], da, C[r]);
          zm = zwm ? h3d_fma(cv.z[0], da, C[r]) : zm;
          zp = zwp ? h3d_fma(cv.z[1], da, C[r]) : zp;
        }
#else
        if constexpr (!FAST) {
          // the mirror ghost: the neighbour across an insulated wall is the centre value
          if (wxm) xm = C[r];
          if (wxp) xp = C[r];
          if ((wyb >> r) & 1) ym = C[r];
          if ((wyb >> (RB + r)) & 1) yp = C[r];
          zm = zwm ? C[r] : zm;
          zp = zwp ? C[r] : zp;
        }
#endif
        // (SW: the rows are the x terms of the update, the marching axis its y terms)
#if H3D_TBL_SRC
        // (the order of the single-step path: wall planes refreshed, then ftcs_update_src)
        const Real nv = add_source<Real>(SW ? ftcs<Real>(C[r], ym, yp, xm, xp, zm, zp, Dx, Dy, Dz)
                                            : ftcs<Real>(C[r], xm, xp, ym, yp, zm, zp, Dx, Dy, Dz),
                                         S[r]);
#else
        const Real nv = SW ? ftcs<Real>(C[r], ym, yp, xm, xp, zm, zp, Dx, Dy, Dz)
                           : ftcs<Real>(C[r], xm, xp, ym, yp, zm, zp, Dx, Dy, Dz);
#endif
#else
        const Real ym = r == 0 ? lo : C[r > 0 ? r - 1 : 0];
        const Real yp = r == NR - 1 ? hi : C[r + 1 < NR ? r + 1 : 0];
        const Real zm = dpp_shr1z(C[r]);
        const Real zp = dpp_shl1z(C[r]);
        // same operation order as kernels.hpp ftcs_update in both frames
#if H3D_TBL_SRC
        const Real nv = add_source<Real>(SW ? ftcs<Real>(C[r], ym, yp, M[r], P[r], zm, zp, Dx, Dy, Dz)
                                            : ftcs<Real>(C[r], M[r], P[r], ym, yp, zm, zp, Dx, Dy, Dz),
                                         S[r]);
#else
        const Real nv = SW ? ftcs<Real>(C[r], ym, yp, M[r], P[r], zm, zp, Dx, Dy, Dz)
                           : ftcs<Real>(C[r], M[r], P[r], ym, yp, zm, zp, Dx, Dy, Dz);
#endif
#endif
        const Real d = resid_abs_r(nv, C[r]);
        bool upd = true, cnt = true, st = true;
        if constexpr (!FAST) {
          upd = xin && ((ybits >> r) & 1);
          cnt = xcnt && ((ybits >> (2 * RB + s * RB + r)) & 1);
          st = xst && ((ybits >> (RB + r)) & 1);
        }
        if (s < K - 1) {
          Real(&N)[RB] = f[s < K - 1 ? s : 0][fw];
          if constexpr (ZSEL) N[r] = zin ? nv : C[r];
          else if constexpr (FAST) N[r] = nv;
          else N[r] = (upd && zin) ? nv : C[r];
        }
        if (!RL || s == K - 1) {
          if constexpr (FAST) {
            // (kStepZ too: cnt has no lane term in any form; the lanes outside
            // the z update range are dropped once, by `ok` at the end)
            m[s] = fmax(m[s], d);
          } else {
            if (cnt) m[s] = fmax(m[s], d);
          }
        }
        if (s == K - 1 && st) {
          // T^{n+K} on the stored region (inside the box, hence the update range)
          nan_seen |= zst && (nv != nv);
          if (zst) buf_store<Real, ST>(nv, plane_rsrc(outw + (int64_t)p * sx), lane_b, r * sy_b);
        }
      }
      if constexpr (Q == 3) {
        // the slot stage 0 has just freed
        if constexpr (!EDGE) {
          if (s == 0) load_plane(x + 2, q[sM]);
        } else {
          if (s == 0) load_rows(x + 2, q[sM], std::integral_constant<int, 0>{}, std::integral_constant<int, NR>{});
        }
      }
    }
  };

  // whole chunks of U steps (the unrolled body needs a constant trip count);
  // padded steps past xlast take the masked form and count / store nothing
  // (without the edge role; with it they are not run)
  // (edge-role kernels: `yfree`, the wave's rows need no y condition.  With
  // zfast that is the mask-free step; in a tile that has columns outside the z
  // update range it is the z-masked step, on the same plane steps [xf_lo, xf_hi],
  // whose bounds hold x terms only.  A padded step past xlast has nothing to
  // count, store or pass on, and no step follows it: the chunk is left there,
  // by every wave of the workgroup alike, so no barrier is left half taken.)
  auto run = [&](auto role_tag, const bool yfree) {
    const bool fast = yfree && zfast, zonly = yfree && !zfast;
    if constexpr (EDGE) {
      // the rings are set up per role: nothing of one role's loop is live in another's
      constexpr int NR = decltype(role_tag)::value ? RB : R;
#pragma unroll
      for (int s = 0; s < K - 1; ++s)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int r = 0; r < NR; ++r) f[s][i][r] = Real(0);
#pragma unroll
      for (int i = 0; i < NPRE; ++i)
        load_rows(x0 - 1 + i, q[i], std::integral_constant<int, 0>{}, std::integral_constant<int, NR>{});
    }
    for (int xb = x0; xb <= xlast; xb += U) {
      static_for<0, U>([&](auto ph_tag) {
        constexpr int ph = decltype(ph_tag)::value;
        const int x = xb + ph;
        if (x > xlast) return;
        const bool xfree = x >= xf_lo && x <= xf_hi;
        if (fast && xfree) step(step_form<kStepFree>{}, x, ph_tag, role_tag);
        else if (zonly && xfree) step(step_form<kStepZ>{}, x, ph_tag, role_tag);
        else step(step_form<kStepMasked>{}, x, ph_tag, role_tag);
      });
    }
  };
  if constexpr (EDGE) {
    // Edge waves: a loop of their own (a role per wave, never per step, keeps
    // the register rows of the other role dead in each loop).  Mask-free
    // where every row is inside the box and the update range: then every
    // cone value is updated, counted and (owned rows, last stage) stored.
    // (The y part of that, and of wfast; run() adds the tile's z part.)
    const bool erows = yb >= max(g.uylo, g.blo[1]) && yb + RB <= min(g.uyhi, g.bhi[1]);
    if (wave == 0) run(std::integral_constant<int, 1>{}, erows);
    else if (wave == WY - 1) run(std::integral_constant<int, 2>{}, erows);
    else run(std::integral_constant<int, 0>{}, wrows);
  } else {
    for (int xb = x0; xb <= xlast; xb += U) {
      static_for<0, U>([&](auto ph_tag) {
        constexpr int ph = decltype(ph_tag)::value;
        const int x = xb + ph;
        if (wfast && x >= xf_lo && x <= xf_hi) step(step_form<kStepFree>{}, x, ph_tag, std::integral_constant<int, 0>{});
        else step(step_form<kStepMasked>{}, x, ph_tag, std::integral_constant<int, 0>{});
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
  if (g.fst) fused_check_tail<K, RL>(g.fst, g.fslot, g.fblocks);
}

