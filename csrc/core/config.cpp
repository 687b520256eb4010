#include "config.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <sstream>

#include <sys/stat.h>

namespace heat3d {

const char* face_name(Face f) {
  static const char* names[] = {"LEFT", "RIGHT", "BOTTOM", "TOP", "BACK", "FRONT"};
  return names[static_cast<int>(f)];
}

const char* dtype_name(DType t) { return t == DType::F64 ? "fp64" : "fp32"; }

DType parse_dtype(const std::string& s) {
  if (s == "fp64" || s == "f64" || s == "double" || s == "float64") return DType::F64;
  if (s == "fp32" || s == "f32" || s == "float" || s == "float32") return DType::F32;
  throw UsageError("unknown dtype '" + s + "' (use fp64 or fp32)");
}

std::string Box::str() const {
  std::ostringstream os;
  os << "[" << lo[0] << "," << hi[0] << ")x[" << lo[1] << "," << hi[1] << ")x[" << lo[2]
     << "," << hi[2] << ")";
  return os.str();
}

Physics Physics::make(int64_t nx, int64_t ny, int64_t nz) {
  Physics p;
  p.n[0] = nx;
  p.n[1] = ny;
  p.n[2] = nz;
  for (int a = 0; a < 3; ++a) {
    HEAT3D_CHECK(p.n[a] >= 3, "grid needs at least 3 vertices per axis, got " << p.n[a]);
    // heat3D.cu:352-355: spacing = L / (N - 1.0)
    p.h[a] = p.length[a] / static_cast<double>(static_cast<double>(p.n[a]) - 1.0);
  }
  const double hmin = std::min({p.h[0], p.h[1], p.h[2]});
  // heat3D.cu:359-360: dt = CFL * 1.0 / (3 * 2) * pow(min(h), 2.0) / alpha
  p.dt = p.cfl * 1.0 / (3 * 2) * std::pow(hmin, 2.0) / p.alpha;
  // heat3D.cu:365-367: D = dt * alpha / pow(h, 2.0)
  for (int a = 0; a < 3; ++a) p.D[a] = p.dt * p.alpha / std::pow(p.h[a], 2.0);
  return p;
}

static const char* const kFaceNames[6] = {"x-", "x+", "y-", "y+", "z-", "z+"};

unsigned parse_insulated(const std::string& s) {
  if (s == "all") return 0x3fu;
  if (s == "none") return 0u;
  unsigned mask = 0;
  std::stringstream ss(s);
  std::string name;
  while (std::getline(ss, name, ',')) {
    int f = -1;
    for (int i = 0; i < 6; ++i)
      if (name == kFaceNames[i]) f = i;
    if (f < 0) throw UsageError("bad --insulated face '" + name + "' (want a list of x-,x+,y-,y+,z-,z+, or all)");
    mask |= 1u << f;
  }
  if (s.empty() || s.back() == ',') throw UsageError("bad --insulated '" + s + "' (want a list of x-,x+,y-,y+,z-,z+, or all)");
  return mask;
}

std::string insulated_str(unsigned mask) {
  std::string out;
  for (int i = 0; i < 6; ++i)
    if ((mask >> i) & 1u) out += (out.empty() ? "" : ",") + std::string(kFaceNames[i]);
  return out.empty() ? "none" : out;
}

static std::string g17(double v) {
  char buf[40];
  std::snprintf(buf, sizeof(buf), "%.17g", v);
  // the shortest of %.15g .. %.17g that reads back as v
  for (int prec = 15; prec < 17; ++prec) {
    char b2[40];
    std::snprintf(b2, sizeof(b2), "%.*g", prec, v);
    if (std::strtod(b2, nullptr) == v) return b2;
  }
  return buf;
}

ConvectiveFaces parse_convective(const std::string& s) {
  ConvectiveFaces out;
  out.fill(-1.0);
  if (s == "none") return out;
  const std::string want = " (want a list of FACE=BETA with FACE one of x-,x+,y-,y+,z-,z+ or all, 0 <= BETA <= 1)";
  if (s.empty() || s.back() == ',') throw UsageError("bad --convective '" + s + "'" + want);
  std::stringstream ss(s);
  std::string item;
  while (std::getline(ss, item, ',')) {
    const auto eq = item.find('=');
    if (eq == std::string::npos) throw UsageError("bad --convective entry '" + item + "'" + want);
    const std::string name = item.substr(0, eq), val = item.substr(eq + 1);
    double beta = 0;
    try {
      size_t pos = 0;
      beta = std::stod(val, &pos);
      if (pos != val.size()) throw std::invalid_argument(val);
    } catch (const std::exception&) {
      throw UsageError("bad --convective coefficient '" + val + "'" + want);
    }
    if (!std::isfinite(beta) || beta < 0.0 || beta > 1.0)
      throw UsageError("--convective coefficient " + val + " of face " + name + " outside [0, 1]" + want);
    if (name == "all") {
      out.fill(beta);
      continue;
    }
    int f = -1;
    for (int i = 0; i < 6; ++i)
      if (name == kFaceNames[i]) f = i;
    if (f < 0) throw UsageError("bad --convective face '" + name + "'" + want);
    out[f] = beta;
  }
  return out;
}

unsigned convective_mask(const ConvectiveFaces& c) {
  unsigned m = 0;
  for (int i = 0; i < 6; ++i)
    if (c[i] >= 0.0) m |= 1u << i;
  return m;
}

std::string convective_str(const ConvectiveFaces& c) {
  std::string out;
  for (int i = 0; i < 6; ++i)
    if (c[i] >= 0.0) out += (out.empty() ? "" : ",") + std::string(kFaceNames[i]) + "=" + g17(c[i]);
  return out.empty() ? "none" : out;
}

std::string ambient_str(double t) { return g17(t); }

std::array<int, 3> parse_decomp(const std::string& s) {
  std::array<int, 3> d = {0, 0, 0};
  int idx = 0;
  std::string cur;
  for (char c : s + "x") {
    if (c == 'x' || c == 'X' || c == ',') {
      if (idx >= 3 || cur.empty()) throw UsageError("bad --decomp '" + s + "' (want AxBxC)");
      d[idx++] = std::atoi(cur.c_str());
      cur.clear();
    } else if (c >= '0' && c <= '9') {
      cur += c;
    } else {
      throw UsageError("bad --decomp '" + s + "' (want AxBxC)");
    }
  }
  if (idx != 3 || d[0] < 1 || d[1] < 1 || d[2] < 1)
    throw UsageError("bad --decomp '" + s + "' (want AxBxC, each >= 1)");
  return d;
}

std::string Config::usage() {
  // Text of heat3D.cu:286-290 followed by the framework's flags.
  std::ostringstream os;
  os << "Incorrect number of command line arguments specified, use the following syntax:\n\n"
     << "bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS\n"
     << "\nor, using MPI, use the following syntax:\n\n"
     << "mpirun -n NUM_PROCS bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS\n"
     << "\nSee source code for additional informations!\n"
     << "\nheat3d (MI355X) options:\n"
     << "  --dtype fp64|fp32         compute precision (default fp64)\n"
     << "  --backend auto|hip|cpu    compute backend (default: hip when a GPU is visible)\n"
     << "  --comm auto|none|local|rccl|socket\n"
     << "                            halo/reduction transport (auto: rccl for multi-process\n"
     << "                            GPU runs, socket for multi-process CPU runs)\n"
     << "  --decomp AxBxC            process grid (default: balanced MPI_Dims_create split)\n"
     << "  --virtual-ranks P         P subdomains in one process (LocalComm)\n"
     << "  --gpus N                  N ranks in this process, one host thread per GPU (RCCL; with\n"
     << "                            --backend cpu: TCP sockets between the threads)\n"
     << "  --device N                GPU ordinal (default LOCAL_RANK)\n"
     << "  --graph / --no-graph      capture iterations in hipGraphs (default on)\n"
     << "  --no-overlap              do not split interior/boundary work\n"
     << "  --check-every K           host poll period of the device convergence flag\n"
     << "  --kernel NAME             single-step kernel (auto|tile[:V:R:WZ:WY:L]|naive)\n"
     << "  --temporal 0|1|K          K-step temporal blocking, K = 2..6 (0 auto: on on the GPU for\n"
     << "                            one subdomain or x slabs; 1 off; results are bitwise identical)\n"
     << "  --kernel2 SPEC            temporally blocked sweep kernel tl2..tl6[:V:R:WZ:WY:L:Q:STORE]\n"
     << "  --output PATH|none        Tecplot output (default output/out.dat for small grids)\n"
     << "  --tecplot-layout auto|ref|owned\n"
     << "  --compat                  reproduce reference reporting quirks\n"
     << "  --scheme ghost|reference  reference: emulate the reference's shared-plane decomposition\n"
     << "                            (edge extrapolation, corner averaging, local norm, any-rank\n"
     << "                            stop; CPU, all ranks of --decomp / --virtual-ranks in-process)\n"
     << "  --checkpoint-every K --checkpoint-dir DIR   periodic binary checkpoints\n"
     << "  --restart DIR             resume from a checkpoint directory\n"
     << "  --source FILE             volumetric heat source q (T_t = alpha lap(T) + q): raw little-endian\n"
     << "                            float64, NX*NY*NZ values, z fastest (the checkpoint field file's order)\n"
     << "  --conductivity FILE       relative conductivity c, 0 < c <= 1 (T_t = div(alpha c grad T) + q), same format\n"
     << "                            as --source; iterations then run as single steps (no K-step sweeps)\n"
     << "  --capacity FILE           relative volumetric heat capacity rc >= 1 (rc T_t = div(alpha c grad T) + q), same\n"
     << "                            format as --source; iterations then run as single steps (no K-step sweeps;\n"
     << "                            not with --compat)\n"
     << "  --insulated FACES         zero-flux (adiabatic) walls: a list of x-,x+,y-,y+,z-,z+ or all; the other\n"
     << "                            faces stay Dirichlet (not with --compat)\n"
     << "  --convective FACE=BETA,.. convective (Robin) walls, -k dT/dn = h (T - T_inf): a list such as y-=0.5,x+=0.25\n"
     << "                            or all=0.5; the neighbour across such a wall is T + BETA (T_inf - T), 0 <= BETA <= 1\n"
     << "                            (BETA = 2 Bi / (2 + Bi), Bi = h * spacing / k; 0 is an insulated wall); a face is\n"
     << "                            Dirichlet, insulated or convective (not with --compat)\n"
     << "  --ambient T               the ambient temperature T_inf of the convective walls (default 0)\n"
     << "  --conductivity-sweeps     with a conductivity field: K-step sweeps of the tv kernels (tv2 / tv3,\n"
     << "                            depth min(K, 3)) instead of single steps; same bits (not with --compat)\n"
     << "  --capacity-sweeps         with a heat capacity and a conductivity field: K-step sweeps of the tc kernels\n"
     << "                            (tc2 / tc3, depth min(K, 3)) instead of single steps; same bits; without a\n"
     << "                            conductivity it does nothing (not with --compat)\n"
     << "  --wall-source-sweeps      with insulated or convective walls and a heat source: K-step sweeps of the\n"
     << "                            wall forms with a source instead of single steps; same bits (not with --compat)\n"
     << "  --heat-balance            after the run report: stored heat, temperature range, heat flow through each\n"
     << "                            face (positive into the body), source power and their balance, summed on the\n"
     << "                            device; also a \"heat_balance\" object in --json-out (not with --compat)\n"
     << "  --steady-solve            solve for the steady state directly instead of stepping in time: conjugate\n"
     << "                            gradients on the device from the initial field; EPS is the relative tolerance\n"
     << "                            of the residual's 2-norm, ITER_MAX caps the iterations; a \"steady_solve\"\n"
     << "                            object in --json-out (fp64 only; not with --compat; needs a Dirichlet face or\n"
     << "                            a convective face with a positive coefficient)\n"
     << "  --implicit M[:THETA]      implicit time steps instead of the explicit time loop: ITER_MAX steps of M\n"
     << "                            explicit time steps each (THETA 1: backward Euler, the default; 0.5: Crank-\n"
     << "                            Nicolson), each solved by conjugate gradients on the device to the relative\n"
     << "                            tolerance EPS; honours --capacity; an \"implicit\" object in --json-out (fp64\n"
     << "                            only; not with --compat or --steady-solve)\n"
     << "  --initial FILE            initial field, same format: its boundary vertices are the fixed wall\n"
     << "                            values, its interior T^0 (the error report still measures against T = y)\n"
     << "  --json-out PATH           write a JSON run report\n"
     << "  --verify-halo K           race detection: checksum every halo face every K iterations\n"
     << "  --timers                  per-phase GPU timing (synchronised diagnostic run)\n"
     << "  --verbose N               print residual every N iterations\n"
     << "  --progress S              stderr heartbeat (iteration, residual, rate) every S seconds of run()\n"
     << "  --time-limit S            run(): stop (not converged) after about S seconds (0 = no limit)\n"
     << "  --threads N               CPU backend OpenMP threads\n"
     << "  --thin-layers             overlapped block sweeps: K-thick y / z boundary layers (default: one\n"
     << "                            tile stride thick, so that their tiles are not mostly halo)\n"
     << "  --reserve-cus N           CUs kept free of the interior sweep for comm / boundary / check\n"
     << "                            kernels (default: 8 = one per XCD when the overlapped\n"
     << "                            multi-rank schedule runs, else 0)\n"
     << "  --lag auto|on|off         lagged convergence check of overlapped sweeps (3rd field buffer)\n"
     << "  --no-block-overlap        block decompositions: exchange the halo first, then sweep\n"
     << "  --no-long-sweeps          step-count remainders as partial sweeps, not K+1-step sweeps\n"
     << "  --long-sweeps auto|on|off remainders as K+1-step sweeps: auto = where the start-up timing of\n"
     << "                            the sweeps finds them cheaper than a partial sweep (default auto;\n"
     << "                            GPU only, measure = on any backend; major = step counts as\n"
     << "                            K+1-step sweeps wherever they fit, as auto does where they are\n"
     << "                            cheaper per step)\n"
     << "  --autotune auto|on|off    time the sweep schedule candidates (z stride, x segments) at start-up;\n"
     << "                            auto: single-subdomain runs (--no-autotune = off)\n"
     << "  --stream-graphs auto|on|off  the overlapped multi-stream schedule as one linear hipGraph per\n"
     << "                            stream with device-side cross-stream waits, verified at start-up\n"
     << "                            (auto = off: eager measured faster on the 8-GPU share; on = graphs;\n"
     << "                            --no-stream-graphs = off)\n"
     << "  --graph-canary S          device-wait timeout of the start-up canary replay of those graphs; a\n"
     << "                            rank whose replay times out or runs > 2x eager turns them off for the\n"
     << "                            job (default 2; 0 = no canary)\n"
     << "  --no-fused-check          single-subdomain sweeps: a check kernel after each sweep instead of\n"
     << "                            the check in the sweep's last workgroup\n"
     << "  --no-monotone-check       fused checks: every step's residual, not only each sweep's last one\n"
     << "                            (the residual max-norm of FTCS never grows, so the last one decides;\n"
     << "                            the converging sweep is replayed with all residuals for the iteration)\n"
     << "  --no-rccl-graph           never record RCCL calls into hipGraphs (eager multi-rank steps)\n"
     << "  --rccl-shared             one RCCL communicator for halos and all-reduces\n"
     << "  --rccl-p2p-channels N     RCCL P2P channel pool (NCCL_MAX_P2P_NCHANNELS unless set in the\n"
     << "                            environment): N > 0 that many; default RCCL's own (8 on the 2-rank\n"
     << "                            one-GPU rehearsal under RCCL 2.27 drove host memory past 270 GB)\n"
     << "  --mem-reserve-gb G        memory preflight reserve (default 2)\n"
     << "  --no-mem-preflight        skip the memory preflight\n"
     << "  --host-mem-limit-gb G     host RAM budget of the gather-to-root Tecplot (default RAM/2)\n"
     << "  --io-stage-mb M           output / checkpoint staging chunk (default 64)\n"
     << "  --watchdog S              abort after S seconds without progress (default 900)\n"
     << "  --fake-allreduce-us U     diagnostic: emulated all-reduce latency for virtual ranks\n"
     << "  --phantom-gbps G --phantom-allreduce-us U --phantom-channels C --phantom-allreduce-channels C\n"
     << "                            phantom-rank proxy (tools/rank_proxy.py) link emulation\n"
     << "  --phantom-wire serial|overlap|paced  phantom exchange: wire time then copies, copies inside it,\n"
     << "                            or copies paced at the wire rate over the wire time\n"
     << "  --phantom-footprint rccl|small  phantom comm kernels in RCCL's kernel footprint (256 threads,\n"
     << "                            140 VGPRs, 20 KB LDS) or small (64 threads; default)\n"
     << "  --quiet                   suppress the banner\n";
  return os.str();
}

static int64_t to_i64(const std::string& s, const char* what) {
  try {
    size_t pos = 0;
    long long v = std::stoll(s, &pos);
    if (pos != s.size()) throw std::invalid_argument(s);
    return v;
  } catch (const std::exception&) {
    throw UsageError(std::string("invalid integer for ") + what + ": '" + s + "'");
  }
}

static double to_f64(const std::string& s, const char* what) {
  try {
    size_t pos = 0;
    double v = std::stod(s, &pos);
    if (pos != s.size()) throw std::invalid_argument(s);
    return v;
  } catch (const std::exception&) {
    throw UsageError(std::string("invalid number for ") + what + ": '" + s + "'");
  }
}

Config Config::parse(int argc, const char* const* argv) {
  Config c;
  if (argc > 0 && argv[0]) c.argv0 = argv[0];
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto need = [&](const char* flag) -> std::string {
      if (i + 1 >= argc) throw UsageError(std::string("missing value for ") + flag);
      return argv[++i];
    };
    // accept --flag=value too
    std::string val;
    auto eq = a.find('=');
    bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
    std::string key = has_eq ? a.substr(0, eq) : a;
    auto get = [&](const char* flag) { return has_eq ? a.substr(eq + 1) : need(flag); };
    if (key.rfind("--", 0) != 0) {
      pos.push_back(a);
      continue;
    }
    if (key == "--dtype") c.dtype = parse_dtype(get("--dtype"));
    else if (key == "--backend") {
      std::string v = get("--backend");
      if (v == "auto") c.backend = BackendKind::Auto;
      else if (v == "hip" || v == "gpu") c.backend = BackendKind::Hip;
      else if (v == "cpu") c.backend = BackendKind::Cpu;
      else throw UsageError("unknown backend '" + v + "'");
    } else if (key == "--comm") {
      std::string v = get("--comm");
      if (v == "auto") c.comm = CommKind::Auto;
      else if (v == "none") c.comm = CommKind::None;
      else if (v == "local") c.comm = CommKind::Local;
      else if (v == "rccl" || v == "nccl") c.comm = CommKind::Rccl;
      else if (v == "socket" || v == "tcp") c.comm = CommKind::Socket;
      else throw UsageError("unknown comm '" + v + "'");
    } else if (key == "--decomp") c.decomp = parse_decomp(get("--decomp"));
    else if (key == "--virtual-ranks") c.virtual_ranks = (int)to_i64(get("--virtual-ranks"), "--virtual-ranks");
    else if (key == "--gpus") c.gpus = (int)to_i64(get("--gpus"), "--gpus");
    else if (key == "--device") c.device = (int)to_i64(get("--device"), "--device");
    else if (key == "--graph") c.use_graph = true;
    else if (key == "--no-graph") c.use_graph = false;
    else if (key == "--overlap") c.overlap = true;
    else if (key == "--no-overlap") c.overlap = false;
    else if (key == "--check-every") c.check_every = (int)to_i64(get("--check-every"), "--check-every");
    else if (key == "--graph-chunk") c.graph_chunk = (int)to_i64(get("--graph-chunk"), "--graph-chunk");
    else if (key == "--kernel") c.kernel = get("--kernel");
    else if (key == "--kernel2") c.kernel2 = get("--kernel2");
    else if (key == "--temporal") {
      c.temporal = (int)to_i64(get("--temporal"), "--temporal");
      if (c.temporal < 0 || c.temporal > 6) throw UsageError("--temporal must be 0 (auto), 1 (off) or 2..6");
    }
    else if (key == "--output") c.output = get("--output");
    else if (key == "--tecplot-layout") c.tecplot_layout = get("--tecplot-layout");
    else if (key == "--compat") c.compat = true;
    else if (key == "--scheme") {
      c.scheme = get("--scheme");
      if (c.scheme != "ghost" && c.scheme != "reference")
        throw UsageError("--scheme must be ghost or reference");
    }
    else if (key == "--checkpoint-every") c.checkpoint_every = to_i64(get("--checkpoint-every"), "--checkpoint-every");
    else if (key == "--verify-halo") c.verify_halo = to_i64(get("--verify-halo"), "--verify-halo");
    else if (key == "--timers") c.timers = true;
    else if (key == "--checkpoint-dir") c.checkpoint_dir = get("--checkpoint-dir");
    else if (key == "--restart") c.restart = get("--restart");
    else if (key == "--source") c.source_file = get("--source");
    else if (key == "--initial") c.initial_file = get("--initial");
    else if (key == "--conductivity") c.conductivity_file = get("--conductivity");
    else if (key == "--capacity") c.capacity_file = get("--capacity");
    else if (key == "--conductivity-sweeps") c.cond_sweeps = true;
    else if (key == "--capacity-sweeps") c.cap_sweeps = true;
    else if (key == "--wall-source-sweeps") c.wall_source_sweeps = true;
    else if (key == "--heat-balance") c.heat_balance = true;
    else if (key == "--steady-solve") c.steady_solve = true;
    else if (key == "--implicit") {
      const std::string v = get("--implicit");
      const auto colon = v.find(':');
      c.implicit = true;
      c.implicit_m = to_f64(v.substr(0, colon), "--implicit");
      c.implicit_theta = colon == std::string::npos ? 1.0 : to_f64(v.substr(colon + 1), "--implicit");
    }
    else if (key == "--insulated") c.insulated = parse_insulated(get("--insulated"));
    else if (key == "--convective") c.convective = parse_convective(get("--convective"));
    else if (key == "--ambient") {
      c.ambient = to_f64(get("--ambient"), "--ambient");
      if (!std::isfinite(c.ambient)) throw UsageError("--ambient must be finite");
    }
    else if (key == "--json-out") c.json_out = get("--json-out");
    else if (key == "--verbose") c.verbose = (int)to_i64(get("--verbose"), "--verbose");
    else if (key == "--progress") c.progress_s = to_f64(get("--progress"), "--progress");
    else if (key == "--time-limit") c.time_limit_s = to_f64(get("--time-limit"), "--time-limit");
    else if (key == "--threads") c.cpu_threads = (int)to_i64(get("--threads"), "--threads");
    else if (key == "--reserve-cus") c.reserve_cus = (int)to_i64(get("--reserve-cus"), "--reserve-cus");
    else if (key == "--quiet") c.quiet = true;
    else if (key == "--lag") {
      const std::string v = get("--lag");
      if (v == "auto") c.lag = -1;
      else if (v == "on" || v == "1") c.lag = 1;
      else if (v == "off" || v == "0") c.lag = 0;
      else throw UsageError("--lag must be auto, on or off");
    }
    else if (key == "--no-block-overlap") c.block_overlap = false;
    else if (key == "--no-long-sweeps") c.long_sweeps = 0;
    else if (key == "--core-rim" || key == "--no-core-rim" || key == "--halo-chunks")
      throw UsageError(key + " was retired in round 5 (measured slower on every configuration, "
                             "profiles/rank_proxy_r04.md)");
    else if (key == "--thin-layers") c.tile_layers = false;
    else if (key == "--boundary-stream")
      throw UsageError("--boundary-stream was retired in round 5 (the boundary pieces run beside the interior "
                       "on the comm stream; after it was slower on every configuration, profiles/r05/proxy_runs.md)");
    else if (key == "--long-sweeps") {
      const std::string v = get("--long-sweeps");
      if (v == "auto") c.long_sweeps = -1;
      else if (v == "on") c.long_sweeps = 1;
      else if (v == "off") c.long_sweeps = 0;
      else if (v == "measure") c.long_sweeps = 2;  // time the sweeps on any backend (tests)
      else if (v == "major") c.long_sweeps = 3;    // measure, and run long-major whatever the timing
      else throw UsageError("--long-sweeps takes auto, on, off, measure or major");
    }
    else if (key == "--no-autotune") c.autotune = 0;
    else if (key == "--autotune") {
      const std::string v = get("--autotune");
      if (v == "auto") c.autotune = -1;
      else if (v == "on") c.autotune = 1;
      else if (v == "off") c.autotune = 0;
      else throw UsageError("--autotune auto|on|off, not '" + v + "'");
    }
    else if (key == "--no-stream-graphs") c.stream_graphs = 0;
    else if (key == "--stream-graphs") {
      const std::string v = get("--stream-graphs");
      if (v != "auto" && v != "on" && v != "off") throw UsageError("--stream-graphs auto|on|off");
      c.stream_graphs = v == "auto" ? -1 : v == "on" ? 1 : 0;
    }
    else if (key == "--graph-canary") c.graph_canary_s = to_f64(get("--graph-canary"), "--graph-canary");
    else if (key == "--no-fused-check") c.fuse_check = false;
    else if (key == "--no-monotone-check") c.monotone_check = false;
    else if (key == "--rccl-graph") c.rccl_graph = true;
    else if (key == "--no-rccl-graph") c.rccl_graph = false;
    else if (key == "--rccl-shared") c.rccl_shared = true;
    else if (key == "--rccl-p2p-channels") c.rccl_p2p_channels = (int)to_i64(get("--rccl-p2p-channels"), "--rccl-p2p-channels");
    else if (key == "--mem-reserve-gb") c.mem_reserve_gb = to_f64(get("--mem-reserve-gb"), "--mem-reserve-gb");
    else if (key == "--no-mem-preflight") c.mem_preflight = false;
    else if (key == "--host-mem-limit-gb") c.host_mem_limit_gb = to_f64(get("--host-mem-limit-gb"), "--host-mem-limit-gb");
    else if (key == "--io-stage-mb") c.io_stage_mb = (int)to_i64(get("--io-stage-mb"), "--io-stage-mb");
    else if (key == "--watchdog") c.watchdog_s = to_f64(get("--watchdog"), "--watchdog");
    else if (key == "--fake-allreduce-us") c.fake_allreduce_us = to_f64(get("--fake-allreduce-us"), "--fake-allreduce-us");
    else if (key == "--phantom-gbps") c.phantom_gbps = to_f64(get("--phantom-gbps"), "--phantom-gbps");
    else if (key == "--phantom-wire") {
      const std::string v = get("--phantom-wire");
      if (v != "serial" && v != "overlap" && v != "paced") throw UsageError("--phantom-wire serial|overlap|paced");
      c.phantom_overlap = v == "overlap";
      c.phantom_paced = v == "paced";
    }
    else if (key == "--phantom-footprint") {
      const std::string v = get("--phantom-footprint");
      if (v != "rccl" && v != "small") throw UsageError("--phantom-footprint rccl|small");
      c.phantom_rccl_footprint = v == "rccl";
    }
    else if (key == "--phantom-allreduce-us")
      c.phantom_allreduce_us = to_f64(get("--phantom-allreduce-us"), "--phantom-allreduce-us");
    else if (key == "--phantom-channels") c.phantom_channels = (int)to_i64(get("--phantom-channels"), "--phantom-channels");
    else if (key == "--phantom-allreduce-channels")
      c.phantom_allreduce_channels = (int)to_i64(get("--phantom-allreduce-channels"), "--phantom-allreduce-channels");
    else if (key == "--help") throw UsageError("help requested");
    else throw UsageError("unknown option '" + a + "'");
  }
  if (pos.size() != 5)
    throw UsageError("expected 5 positional arguments (NX NY NZ ITER_MAX EPS), got " +
                     std::to_string(pos.size()));
  c.n[0] = to_i64(pos[0], "NUM_CELLS_X");
  c.n[1] = to_i64(pos[1], "NUM_CELLS_Y");
  c.n[2] = to_i64(pos[2], "NUM_CELLS_Z");
  c.iter_max = to_i64(pos[3], "ITER_MAX");
  c.eps = to_f64(pos[4], "EPS");
  c.eps_text = pos[4];
  for (int a = 0; a < 3; ++a)
    if (c.n[a] < 3) throw UsageError("each grid extent must be >= 3");
  if (c.iter_max < 0) throw UsageError("ITER_MAX must be >= 0");
  if (c.virtual_ranks < 1) throw UsageError("--virtual-ranks must be >= 1");
  if (c.gpus < 0) throw UsageError("--gpus must be >= 1");
  if (c.gpus > 1 && c.virtual_ranks > 1) throw UsageError("--gpus and --virtual-ranks are exclusive");
  if (c.check_every < 1) c.check_every = 1;
  if (c.graph_chunk < 0) c.graph_chunk = 0;
  if (c.graph_chunk == 1) c.graph_chunk = 2;
  if (c.graph_chunk % 2) c.graph_chunk += 1;
  if (c.io_stage_mb < 1) c.io_stage_mb = 1;
  if (c.watchdog_s <= 0) throw UsageError("--watchdog must be > 0");
  if (c.progress_s < 0) throw UsageError("--progress must be >= 0");
  if (c.time_limit_s < 0) throw UsageError("--time-limit must be >= 0");
  // --source / --initial / --conductivity / --capacity: NX*NY*NZ float64 values; a wrong size is a usage error
  for (const auto* f : {&c.source_file, &c.initial_file, &c.conductivity_file, &c.capacity_file}) {
    if (f->empty()) continue;
    const char* flag = f == &c.source_file         ? "--source"
                       : f == &c.initial_file      ? "--initial"
                       : f == &c.conductivity_file ? "--conductivity"
                                                   : "--capacity";
    struct stat st {};
    if (::stat(f->c_str(), &st) != 0) throw UsageError(std::string(flag) + ": cannot read file " + *f);
    const long long want = (long long)c.n[0] * c.n[1] * c.n[2] * 8;
    if ((long long)st.st_size != want)
      throw UsageError(std::string(flag) + " file " + *f + " has " + std::to_string((long long)st.st_size) +
                       " bytes, expected " + std::to_string(want) + " (NX*NY*NZ little-endian float64 values)");
  }
  if (!c.initial_file.empty() && !c.restart.empty()) throw UsageError("--initial and --restart are exclusive");
  if ((!c.source_file.empty() || !c.initial_file.empty() || !c.conductivity_file.empty()) && c.scheme == "reference")
    throw UsageError("--source / --initial / --conductivity are not part of --scheme reference");
  if (!c.conductivity_file.empty() && c.compat)
    throw UsageError("--conductivity is not part of --compat (the reference's uniform material)");
  if (!c.capacity_file.empty() && (c.compat || c.scheme == "reference"))
    throw UsageError("--capacity is not part of --compat / --scheme reference (the reference's uniform material)");
  if (c.insulated && (c.compat || c.scheme == "reference"))
    throw UsageError("--insulated is not part of --compat / --scheme reference (the reference's Dirichlet walls)");
  if (convective_mask(c.convective) && (c.compat || c.scheme == "reference"))
    throw UsageError("--convective is not part of --compat / --scheme reference (the reference's Dirichlet walls)");
  if (convective_mask(c.convective) & c.insulated)
    throw UsageError("a face is either insulated or convective: --insulated " + insulated_str(c.insulated) +
                     " and --convective " + convective_str(c.convective) + " share " +
                     insulated_str(convective_mask(c.convective) & c.insulated));
  if (c.cond_sweeps && c.compat)
    throw UsageError("--conductivity-sweeps is not part of --compat (the reference's uniform material)");
  if (c.cap_sweeps && c.compat)
    throw UsageError("--capacity-sweeps is not part of --compat (the reference's uniform material)");
  if (c.heat_balance && (c.compat || c.scheme == "reference"))
    throw UsageError("--heat-balance is not part of --compat / --scheme reference (the reference's report)");
  if (c.steady_solve) {
    if (c.compat || c.scheme == "reference")
      throw UsageError("--steady-solve is not part of --compat / --scheme reference (the reference only steps in time)");
    if (c.dtype != DType::F64)
      throw UsageError("--steady-solve needs --dtype fp64: in fp32 conjugate gradients cannot get below about "
                       "kappa * 2^-24 (kappa ~ 4e5 at 1024^3)");
    if (!(c.eps > 0.0))
      throw UsageError("--steady-solve: EPS is the relative tolerance and must be positive");
    bool anchored = false;
    for (int f = 0; f < kNumFaces; ++f)
      anchored |= c.convective[f] > 0.0 || (c.convective[f] < 0.0 && !((c.insulated >> f) & 1u));
    if (!anchored)
      throw UsageError("--steady-solve needs a Dirichlet face or a convective face with a positive coefficient: "
                       "with every face insulated the system is singular");
  }
  if (c.implicit) {
    if (c.steady_solve) throw UsageError("--implicit and --steady-solve exclude each other");
    if (c.compat || c.scheme == "reference")
      throw UsageError("--implicit is not part of --compat / --scheme reference (the reference's explicit step)");
    if (c.dtype != DType::F64)
      throw UsageError("--implicit needs --dtype fp64: in fp32 conjugate gradients cannot get below about kappa * 2^-24");
    if (!(c.implicit_m > 0.0) || !std::isfinite(c.implicit_m))
      throw UsageError("--implicit: M, the step length in explicit time steps, must be positive and finite");
    if (!(c.implicit_theta >= 0.5 && c.implicit_theta <= 1.0))
      throw UsageError("--implicit: THETA must lie in [0.5, 1] (1: backward Euler, 0.5: Crank-Nicolson)");
    if (!(c.eps > 0.0) || !std::isfinite(c.eps))
      throw UsageError("--implicit: EPS is the relative tolerance of each step's solve and must be positive");
  }
  if (c.wall_source_sweeps && c.compat)
    throw UsageError("--wall-source-sweeps is not part of --compat (the reference has neither walls nor a source)");
  return c;
}

std::string Config::echo_banner() const {
  // heat3D.cu:293-302 (including the "Runnung" typo and trailing space, B.4).
  std::ostringstream os;
  os << "Runnung HeatEquation3D with the following arguments: \n";
  os << "executable:               " << argv0 << "\n";
  os << "number of cells in x:     " << n[0] << "\n";
  os << "number of cells in y:     " << n[1] << "\n";
  os << "number of cells in z:     " << n[2] << "\n";
  os << "max number of iterations: " << iter_max << "\n";
  os << "convergence threshold:    " << eps << "\n";
  if (convective_mask(convective)) {
    os << "convective walls:         " << convective_str(convective) << "\n";
    os << "ambient temperature:      " << ambient_str(ambient) << "\n";
  }
  os << "\n";
  return os.str();
}

}  // namespace heat3d
