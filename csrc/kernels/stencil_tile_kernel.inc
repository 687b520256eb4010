// heat3d-mi355x — the single-step tile kernel's definition, included by
// kernels_hip.hip once per form: H3D_TILE_NAME stencil_tile with H3D_TILE_SRC 0,
// and stencil_tile_src with H3D_TILE_SRC 1 (the update adds the heat source S,
// kernels.hpp ftcs_update_src).  Textual inclusion keeps the kernel without a
// source exactly the code it was before the source form existed.
template <typename Real, int V, int R, int WZ, int WY>
__global__ __launch_bounds__(64 * WZ * WY) void H3D_TILE_NAME(const Real* __restrict__ in,
                                                             Real* __restrict__ out,
#if H3D_TILE_SRC
                                                             const Real* __restrict__ src,
#endif
                                                             Layout L,
                                                             Box b, TileGeom g, Real Dx, Real Dy,
                                                             Real Dz, unsigned long long* res,
                                                             const int* done) {
  typedef typename VecOf<Real, V>::type Vec;
  constexpr int TZ = 64 * V;
  constexpr int NW = WZ * WY;
  // [parity][wave][bottom/top row][lane]
  __shared__ Vec s_rows[2][NW][2][64];
  // [parity][wave][row][left/right]
  __shared__ Real s_edge[2][NW][R][2];
  if (flag_set(done)) return;  // uniform across the block

  const int blk = blockIdx.x;
  const int xcd = blk & 7;
  int64_t t = xcd * g.xq + min(xcd, g.xr) + (blk >> 3);
  const int zb = (int)(t % g.nzb);
  t /= g.nzb;
  const int ybk = (int)(t % g.nyb);
  const int xs = (int)(t / g.nyb);

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wz = wave % WZ, wy = wave / WZ;
  const int64_t kb = g.z0a + ((int64_t)zb * WZ + wz) * TZ;
  const int64_t k = kb + (int64_t)lane * V;
  const int64_t yb = b.lo[1] + ((int64_t)ybk * WY + wy) * R;
  const int ract = (int)max((int64_t)0, min((int64_t)R, b.hi[1] - yb));
  // neighbours in the tile: below (wy-1) always has R rows; above only if I am full
  const bool nb_lo = wy > 0;
  const bool nb_hi = (wy + 1 < WY) && (ract == R) && (yb + R < b.hi[1]);
  const bool nb_left = wz > 0, nb_right = wz + 1 < WZ;
  const int64_t xa = b.lo[0] + (int64_t)xs * g.seg;
  const int64_t xe = min(xa + (int64_t)g.seg, b.hi[0]);
  const int64_t sx = L.sx, sy = L.sy;

  bool valid[V];
  bool allvalid = true;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    valid[v] = (k + v >= b.lo[2]) && (k + v < b.hi[2]);
    allvalid &= valid[v];
  }
  const int64_t base0 = L.index(0, yb, k);
  // outer-edge gather: lanes [0,R) left edges (only the wz == 0 wave), lanes
  // [32,32+R) right edges (only the wz == WZ-1 wave)
  const int er = lane < 32 ? lane : lane - 32;
  const bool eload = er < ract && (lane < 32 ? !nb_left : !nb_right);
  const int64_t ebase = L.index(0, yb + er, lane < 32 ? kb - 1 : kb + TZ);

  auto ld = [&](int64_t plane, int r) -> Vec {
    return *reinterpret_cast<const Vec*>(in + base0 + plane * sx + (int64_t)r * sy);
  };

  Vec qm[R], qc[R], qp[R];
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r < ract) {
      qm[r] = ld(xa - 1, r);
      qc[r] = ld(xa, r);
      qp[r] = ld(xa + 1, r);
    }
  Vec hb = {}, ht = {};
  if (ract > 0 && !nb_lo) hb = ld(xa, -1);
  if (ract > 0 && !nb_hi) ht = ld(xa, ract);
  Real ed = eload ? in[ebase + xa * sx] : Real(0);

  double m = 0.0;
  int par = 0;
  for (int64_t x = xa; x < xe; ++x) {
    // publish this wave's boundary rows / edge points of plane x
    if (ract > 0) {
      s_rows[par][wave][0][lane] = qc[0];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r == ract - 1) s_rows[par][wave][1][lane] = qc[r];  // static register index
        if (r < ract) {
          if (lane == 0) s_edge[par][wave][r][0] = qc[r][0];
          if (lane == 63) s_edge[par][wave][r][1] = qc[r][V - 1];
        }
      }
    }
    // prefetch plane x+2 centres and plane x+1 outer halo
    Vec qn[R];
    Vec hbn = {}, htn = {};
    Real edn = Real(0);
    const bool more = x + 1 < xe;
    if (more && ract > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (r < ract) qn[r] = ld(x + 2, r);
      if (!nb_lo) hbn = ld(x + 1, -1);
      if (!nb_hi) htn = ld(x + 1, ract);
      if (eload) edn = in[ebase + (x + 1) * sx];
    }
    __syncthreads();
    if (ract > 0) {
      const Vec ylo = nb_lo ? s_rows[par][wave - WZ][1][lane] : hb;
      const Vec yhi = nb_hi ? s_rows[par][wave + WZ][0][lane] : ht;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < ract) {
          const Vec c = qc[r];
#if H3D_TILE_SRC
          // the source row (same layout, same vector load as the field's)
          const Vec sv = *reinterpret_cast<const Vec*>(src + base0 + x * sx + (int64_t)r * sy);
#endif
          const Vec ym = r == 0 ? ylo : qc[r > 0 ? r - 1 : 0];
          const Vec yp = (r == ract - 1) ? yhi : qc[r + 1 < R ? r + 1 : R - 1];
          const Real left = nb_left ? s_edge[par][wave - 1][r][1] : readlane(ed, r);
          const Real right = nb_right ? s_edge[par][wave + 1][r][0] : readlane(ed, 32 + r);
          Vec zm, zp, nv;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            zm[v] = v == 0 ? dpp_shr1(left, c[V - 1]) : c[v > 0 ? v - 1 : 0];
            zp[v] = v == V - 1 ? dpp_shl1(right, c[0]) : c[v + 1 < V ? v + 1 : 0];
          }
#pragma unroll
          for (int v = 0; v < V; ++v) {
            nv[v] = ftcs<Real>(c[v], qm[r][v], qp[r][v], ym[v], yp[v], zm[v], zp[v], Dx, Dy, Dz);
#if H3D_TILE_SRC
            nv[v] = add_source<Real>(nv[v], sv[v]);
#endif
            if (valid[v]) m = res_max(m, resid_abs(nv[v], c[v]));
          }
          Real* dst = out + base0 + x * sx + (int64_t)r * sy;
          if (allvalid) {
            if (g.nt) __builtin_nontemporal_store(nv, reinterpret_cast<Vec*>(dst));
            else *reinterpret_cast<Vec*>(dst) = nv;
          } else {
#pragma unroll
            for (int v = 0; v < V; ++v)
              if (valid[v]) dst[v] = nv[v];
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      qm[r] = qc[r];
      qc[r] = qp[r];
      qp[r] = qn[r];
    }
    hb = hbn;
    ht = htn;
    ed = edn;
    par ^= 1;
  }
  if (res) residual_commit(res, m);
}

