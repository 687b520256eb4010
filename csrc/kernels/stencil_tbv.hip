// heat3d-mi355x — K-step temporally blocked sweeps with a spatially varying
// conductivity ("tv"): T_t = div(kappa grad T) + q, K time steps per HBM sweep.
//
// Same contract as the lean kernel (stencil_tbl_impl.hpp): one sweep turns T^n
// into T^{n+K} on p.box, the intermediate stages are computed on the update
// ranges, stage s records its residual in slot p.slot + s over the counting
// region of cpu::stencil_multi, and every point goes through the update of
// kernels.hpp, here ftcs_update_varw, so fields and residuals are bitwise those
// of K single steps with p.cond.  The geometry is the lean kernel's: 64-lane
// tiles storing up to 64 - 2K columns, WY waves of R rows marching x, a T^n ring
// of three planes, stage rings f[K-1][3][R], one LDS barrier per plane step for
// the y edge rows of every stage's centre plane, zero-fill DPP shifts for z,
// buffer loads with SGPR row offsets clamped to the live rows and planes.
//
// What is new is the static field Ch = dtype(0.5 c).  Stage s at step x works
// on plane x - s and reads Ch on planes x - s - 1 .. x - s + 1, so one register
// ring of the planes x - K .. x + 1, loaded once per plane step (two planes
// ahead, one at K = 4), serves every stage.  A wave keeps R + 2 rows of
// every Ch plane: its own and the two y neighbours of its edge rows, loaded
// directly (Ch is static; the neighbouring wave and tile load the same rows, so
// these are cache hits) instead of a second LDS exchange, for which the LDS of
// a 16-wave tile has no room.  Every face weight is formed where it is used, as
// the one rounded add Ch[p] + Ch[q]: the add commutes, so both cells of a face
// get the same bits, and the operands are exactly those ftcs_update_var adds on
// the CPU.  z neighbours of Ch come by the same zero-fill DPP as T's: lanes 0
// and 63 are outside every stage's cone.  Ch loads are clamped exactly as the T
// loads are; a clamped value only ever feeds a masked-out result.
//
// Out of scope here (the lean kernel has them): the fused convergence check,
// schedule tuning, last-residual-only variants, packed pairs, the edge role and
// the y-marching thin-slab forms.  Thin boxes are correct, not fast.
#include "stencil_tbl_impl.hpp"

namespace heat3d {
namespace hip {

namespace {

// Ch ring: 6 slots for every depth (lcm(3, 6, 2) = 6 keeps the unroll that makes
// the ring indices static short; a slot no stage reads costs no register), and
// how many planes ahead of step x the ring is loaded
constexpr int kTbvRing = 6;
constexpr int tbv_ahead(int K) { return K <= 3 ? 2 : 1; }

}  // namespace

template <typename Real, int R, int WY, int K, bool SRC>
__global__ __launch_bounds__(64 * WY) void stencil_tbv(const Real* __restrict__ in, Real* __restrict__ out,
                                                       const Real* __restrict__ ch, const Real* __restrict__ src,
                                                       TBLArgs g, Real Dx, Real Dy, Real Dz,
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
  const bool zfast = c0 >= g.uzlo && c0 + 64 <= g.uzhi;
  const bool wrows = tr0 >= K && tr0 + R <= TY - K && yb >= g.uylo && yb + R <= g.uyhi && yb >= g.blo[1] &&
                     yb + R <= g.bhi[1];
  const bool wfast = zfast && wrows;
  // steps whose every stage is valid, updated, counted and (last stage) stored
  const int xf_lo = max(max(x0 + 2 * (K - 1), g.ulo + K - 1), g.blo[0] + K - 1);
  const int xf_hi = min(min(xlast, g.uhi - 1), g.bhi[0] + K - 2);

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

  // ---- addressing: uniform bases, clamped row offsets (all >= 0: clamping is
  // monotonic).  The Ch rows start one row earlier: row -1 of the wave.
  auto yclamp = [&](int row) { return min(max(row, g.ylo_live), g.yhi_live); };
  const int ybc = yclamp(yb), ybm = yclamp(yb - 1);
  const Real* __restrict__ inw = in + (g.origin + (int64_t)ybc * g.sy + c0);
  const Real* __restrict__ chw = ch + (g.origin + (int64_t)ybm * g.sy + c0);
  Real* __restrict__ outw = out + (g.origin + (int64_t)yb * g.sy + c0);
  const Real* __restrict__ srcw = SRC ? src + (g.origin + (int64_t)ybc * g.sy + c0) : nullptr;
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
      // masked form: uniform x conditions of this stage
      bool xin = true, xcnt = true, xst = true;
      if constexpr (!FAST) {
        xin = p >= g.ulo && p < g.uhi;
        xcnt = xin && x >= x0 + 2 * s && x <= xlast && p >= g.blo[0] - (K - 1 - s) && p < g.bhi[0] + (K - 1 - s);
        xst = p >= xa && p < xe;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const Real ym = r == 0 ? lo : C[r > 0 ? r - 1 : 0];
        const Real yp = r == R - 1 ? hi : C[r + 1 < R ? r + 1 : 0];
        const Real zm = dpp_shr1z(C[r]);
        const Real zp = dpp_shl1z(C[r]);
        const Real hc = HC[r + 1];
        // the six face weights, each the one rounded add of ftcs_update_var
        const Real wxm = hc + HM[r + 1], wxp = hc + HP[r + 1];
        const Real wym = hc + HC[r], wyp = hc + HC[r + 2];
        const Real wzm = hc + dpp_shr1z(hc), wzp = hc + dpp_shl1z(hc);
        Real nv = ftcs_update_varw<Real>(C[r], M[r], P[r], ym, yp, zm, zp, wxm, wxp, wym, wyp, wzm, wzp, Dx, Dy, Dz);
        if constexpr (SRC) nv = add_source<Real>(nv, S[r]);
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

template <typename Real, int R, int WY, int K, bool SRC>
static void launch_tbv(const StencilParams& p, const KernelSpec& ks, hipStream_t s) {
  const void* kfn = reinterpret_cast<const void*>(&stencil_tbv<Real, R, WY, K, SRC>);
  const Box& b = p.box;
  const Layout& L = p.L;
  constexpr int TY = WY * R;
  HEAT3D_CHECK(L.n[0] + 2 * L.gx < (1LL << 30) && L.n[1] + 2 * L.gy < (1LL << 30) &&
                   L.sy * (int64_t)sizeof(Real) * (R + 2 + 2 * L.gy + TY + 2 * K) < (1LL << 31),
               "tv: extents exceed 32-bit tile coordinates");
  TBLArgs g{};
  g.sx = L.sx;
  g.sy = L.sy;
  g.origin = L.origin;
  for (int a = 0; a < 3; ++a) {
    g.blo[a] = (int)b.lo[a];
    g.bhi[a] = (int)b.hi[a];
  }
  const bool wx = p.ux[1] >= p.ux[0], wy = p.uy[1] >= p.uy[0], wz = p.uz[1] >= p.uz[0];
  g.ulo = (int)(wx ? p.ux[0] : b.lo[0]);
  g.uhi = (int)(wx ? p.ux[1] : b.hi[0]);
  g.uylo = (int)(wy ? p.uy[0] : b.lo[1]);
  g.uyhi = (int)(wy ? p.uy[1] : b.hi[1]);
  g.uzlo = (int)(wz ? p.uz[0] : b.lo[2]);
  g.uzhi = (int)(wz ? p.uz[1] : b.hi[2]);
  g.xlo_live = (int)-L.gx;
  g.xhi_live = (int)(L.n[0] + L.gx - 1);
  g.ylo_live = (int)-L.gy;
  g.yhi_live = (int)(L.n[1] + L.gy - 1);
  // every loaded column of every tile lies inside the row's allocation (as the
  // lean kernel: rows start zoff >= 16 elements before k = 0, the tail pad
  // covers the last tile's overhang); the store box is owned points
  HEAT3D_CHECK(b.lo[2] - K >= -L.zoff, "tv: tile columns before the row start");
  for (int a = 0; a < 3; ++a)
    HEAT3D_CHECK(b.lo[a] >= 0 && b.hi[a] <= L.n[a], "tv: box " << b.str() << " outside the owned extents");
  HEAT3D_CHECK(g.uylo - 1 >= -L.gy && g.uyhi <= L.n[1] + L.gy && g.uylo <= b.lo[1] && g.uyhi >= b.hi[1] &&
                   g.uzlo - 1 >= -L.gz && g.uzhi <= L.n[2] + L.gz && g.uzlo <= b.lo[2] && g.uzhi >= b.hi[2],
               "tv: y/z update range outside the ghosted layout");
  HEAT3D_CHECK(g.ulo - 1 >= g.xlo_live && g.uhi <= g.xhi_live + 1 && g.ulo <= b.lo[0] && g.uhi >= b.hi[0],
               "tv: u range [" << g.ulo << "," << g.uhi << ") outside the ghosted layout");
  constexpr int YS = TY - 2 * K;
  constexpr int U = lcm_l(lcm_l(kTbvRing, 3), 2);  // the kernel's unroll
  static const int slots = device_slots(kfn, 64 * WY);
  const int ZS = ks.ZS > 0 ? ks.ZS : 64 - 2 * K;
  HEAT3D_CHECK(ZS >= 1 && ZS <= 64 - 2 * K, "tv: z stride " << ZS << " outside [1, " << 64 - 2 * K << "]");
  g.c00 = (int)(b.lo[2] - K);
  g.r00 = (int)(b.lo[1] - K);
  g.nyb = (int)std::max<int64_t>(1, (b.extent(1) + YS - 1) / YS);
  g.zs = ZS;
  g.nzb = (int)std::max<int64_t>(1, (b.extent(2) + ZS - 1) / ZS);
  const int64_t tiles = (int64_t)g.nzb * g.nyb;
  const int64_t nxb = b.extent(0);
  HEAT3D_CHECK(!p.state || p.slot + K <= kResidualSlots, "tv: residual slots " << p.slot << "+" << K);
  auto scratch = [](const void* f) {
    hipFuncAttributes a{};
    return hipFuncGetAttributes(&a, f) == hipSuccess ? (int)a.localSizeBytes : 0;
  };
  static const int spill = scratch(kfn);
  HEAT3D_CHECK(spill == 0, "tv variant " << ks.str() << " spills " << spill << " B of registers per lane");
  unsigned long long* r = p.state && p.residual ? &p.state->residual[p.slot] : nullptr;
  const int* done = p.state ? &p.state->done : nullptr;
  const XPlan xp = ks.L > 0 ? fixed_xplan(nxb, tiles, ks.L) : plan_x(nxb, tiles, slots, 2 * (K - 1), U, ks.L == -1);
  HEAT3D_CHECK(xp.seg >= 1 && xp.seg < (1 << 15) && xp.split < (1 << 15) && xp.r < (1 << 30), "tv: x plan out of range");
  g.segsplit = xp.seg | (xp.split << 16);
  g.n1 = xp.n1;
  g.rb = xp.r | (xp.nb2 > 0 ? (1 << 30) : 0);
  const int64_t nblocks = (int64_t)xp.n1 + xp.r + xp.nb2;
  HEAT3D_CHECK(nblocks < (1LL << 31) && nblocks >= 1, "tv: bad block count " << nblocks);
  if (trace_enabled())
    std::fprintf(stderr, "[heat3d trace] tv K=%d box x %lld: zs=%d seg=%d tiles=%dx%d blocks=%lld\n", K, (long long)nxb,
                 ZS, xp.seg, g.nzb, g.nyb, (long long)nblocks);
  hipLaunchKernelGGL((stencil_tbv<Real, R, WY, K, SRC>), dim3((unsigned)nblocks), dim3(64 * WY), 0, s,
                     static_cast<const Real*>(p.in), static_cast<Real*>(p.out), static_cast<const Real*>(p.cond),
                     static_cast<const Real*>(p.src), g, (Real)p.D[0], (Real)p.D[1], (Real)p.D[2], r, done);
  HIPK_CHECK(hipGetLastError());
}

// One shape per (dtype, K), with and without a heat source (register report:
// profiles/cond_sweeps.md).  p == nullptr: only report whether the form exists.
template <typename Real>
static bool dispatch_tbv(const StencilParams* p, const KernelSpec& k, hipStream_t s) {
  if (k.V || k.R || k.WZ || k.WY || k.NT || k.O > 0 || k.EW) return false;  // no shape fields
  const bool q = p && p->src;
#define H3D_TBV(RR, YY, KK)                                      \
  if (k.K == KK) {                                               \
    if (p && q) launch_tbv<Real, RR, YY, KK, true>(*p, k, s);    \
    else if (p) launch_tbv<Real, RR, YY, KK, false>(*p, k, s);   \
    return true;                                                 \
  }
  if constexpr (sizeof(Real) == 8) {
    // 16 waves of 2 rows (128 VGPRs); K = 3: 12 waves (168).  Three rows per
    // wave spill at either depth, and no fp64 K = 4 shape of >= 8 waves fits
    H3D_TBV(2, 16, 2)
    H3D_TBV(2, 12, 3)
  } else {
    H3D_TBV(5, 16, 2)
    H3D_TBV(4, 12, 3)
  }
#undef H3D_TBV
  return false;
}

bool cond_sweep_supported(DType t, const KernelSpec& k, bool /*with_source*/) {
  if (k.kind != KernelSpec::TBV) return false;
  return t == DType::F64 ? dispatch_tbv<double>(nullptr, k, nullptr) : dispatch_tbv<float>(nullptr, k, nullptr);
}

int cond_sweep_max_depth(DType t) {
  KernelSpec k;
  k.kind = KernelSpec::TBV;
  int best = 0;
  for (k.K = 2; k.K <= 6; ++k.K)
    if (cond_sweep_supported(t, k, false)) best = k.K;
  return best;
}

void stencil_cond_sweep(DType t, const StencilParams& p, const KernelSpec& k, void* stream) {
  HEAT3D_CHECK(k.kind == KernelSpec::TBV, "stencil_cond_sweep needs a tv kernel");
  if (!p.cond) HEAT3D_THROW("tv kernels need a conductivity field (" << k.str() << " without one; use tl2..tl6)");
  HEAT3D_CHECK(!p.fuse_check && !p.tune, "tv kernels have no fused check and no schedule tuning");
  if (p.box.empty()) return;
  const bool ok = t == DType::F64 ? dispatch_tbv<double>(&p, k, S(stream)) : dispatch_tbv<float>(&p, k, S(stream));
  if (!ok)
    HEAT3D_THROW("unsupported tv kernel variant " << k.str() << " (" << dtype_name(t)
                                                  << "): tv2 and tv3, without shape fields");
}

}  // namespace hip
}  // namespace heat3d
