// The device code that mp_lift_fit_skeleton (lift_skeleton.hip) and mp_lift_fit_skeleton_smooth (lift_skeleton_smooth.hip) share: a frame's
// arguments and LDS, the evaluation (rule 3), one Gauss-Newton step (rules 4 to 8), the per-frame fit (rules 0 to 10) and the host's argument
// checks.  Included after `#pragma clang fp contract(off)` and lift_geom.h: the code takes the including file's floating-point mode.
//
// ONE 64-LANE WORKGROUP (one wave) OWNS ONE FRAME: a coupled system of up to 65 unknowns does not fit a lane.  Lane j evaluates joint j (the
// view loop unrolled to MP_LIFT_FUSE_MAXV, as lift_triangulate.hip's tri_eval: rotation re-made from the quaternion, nothing in a register array)
// into a per-joint 3x3 S_j and g_j in LDS; the subtree sums run joint by joint from the leaves, one lane per matrix entry; lane b forms bone
// b's tangent basis, its M_b = T B and the two rows of H that belong to its unknowns (the blocks with its ancestors; a host-built bit mask per
// bone says which); the packed lower triangle of H is factorised column by column, every lane the pivot, the lanes striding over the column's
// rows, one barrier per column; lane 0 substitutes.  The dense 3 x U Jacobian is never formed.  Everything indexed at run time is LDS or a kernel
// argument (parents, ancestor masks).  Every decision is computed by every lane from the same LDS values or by a wave vote, so control is uniform.
// The rotation, the view test, the projection with its Jacobian, the 3x3 normal equations and the accept rule are lift_geom.h's.
// Everything between the float32 loads and the float32 stores is fp64, without contraction; no atomics, fixed orders: identical bits on every call.
#pragma once

namespace mp {

constexpr int SK_MAXV = MP_LIFT_FUSE_MAXV;
constexpr int SK_THREADS = 64;                          // one wave: the votes below (__all, __any) span the workgroup
constexpr int SK_MAXB = LIFT_MAXJ - 1;                  // bones
constexpr int SK_MAXU = 3 + 2 * SK_MAXB;                // unknowns: 65, one more than the wave - every loop over them strides
constexpr int SK_TRI = SK_MAXU * (SK_MAXU + 1) / 2;     // the packed lower triangle: 2145 doubles
constexpr double SK_PIVOT = 1e-12;                      // lift_bundle.hip's BUNDLE_PIVOT rule
constexpr double SK_DIR = 1e-12;                        // a start bone shorter than this has no direction of its own

struct SkelArgs {
  const float* start;            // (Ftot, J, 3)
  const unsigned char* start_ok; // (Ftot) or null
  const float* kp;               // (V, Ftot, J, 2)
  const float* kp_weight;        // (V, Ftot, J) or null
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* quat;             // (G, V, 4)
  const float* trans;            // (G, V, 3)
  const float* intr;             // (G, V, 9)
  const float* lengths;          // (G, J - 1)
  float* pose;                   // (Ftot, J, 3)
  float* err;                    // (Ftot, 2); (Ftot, 3) for mp_lift_fit_skeleton_smooth
  unsigned char* ok;             // (Ftot)
  unsigned char* steps;          // (Ftot) or null
  long Ftot;
  double sigma2, prior;
  int V, J, G, distort, iters;
  signed char parent[LIFT_MAXJ];
  unsigned anc[SK_MAXB];         // bit a of anc[b]: bone a is b or lies on the path from the root to b
  // what mp_lift_fit_skeleton_smooth adds (at the end: nothing above moves): a frame's fp64 state between the launches,
  // (r, d_0 .. d_{J-2}, p_0 .. p_{J-1}), 6 J doubles a frame
  double* state;                 // (Ftot, 6 J)
  unsigned char* moves;          // (Ftot) or null
};

struct SkelLds {
  double H[SK_TRI];                                     // the system's lower triangle, packed by rows; below the diagonal it becomes the factor
  double diag[SK_MAXU], rhs[SK_MAXU], x[SK_MAXU];       // the factor's diagonal, the right side, the solution
  double S[LIFT_MAXJ][6], g[LIFT_MAXJ][3];              // per joint (H00 H01 H02 H11 H12 H22) and g, then the subtree sums in place
  double Fj[LIFT_MAXJ], Ej[LIFT_MAXJ], Wj[LIFT_MAXJ];
  double p[2][LIFT_MAXJ][3];                            // two slots: the state and the candidate
  double r[2][3], d[2][SK_MAXB][3];
  double e1[SK_MAXB][3], e2[SK_MAXB][3], B[SK_MAXB][6], M[SK_MAXB][6];    // B, M (3x2): entry (i, c) at 2 i + c
  double len[SK_MAXB];
  int own[SK_MAXB];
};

__device__ __forceinline__ int sk_idx(int i, int k) { return i * (i + 1) / 2 + k; }   // i >= k

// entry (i, k) of the symmetric 3x3 kept as (00 01 02 11 12 22)
__device__ __forceinline__ double sk_sym(const double* s, int i, int k) {
  const int a = i < k ? i : k, b = i < k ? k : i;
  return s[a == 0 ? b : (a == 1 ? 2 + b : 5)];
}

struct SkelCost { double F, E, W; bool deep; };

// the second pull of a visit of mp_lift_fit_skeleton_smooth: lam = smooth W_t, and lane j's q_j
struct SkelPull { double lam, x, y, z; };

// 3. of the rule at slot c's (r, d): the positions in joint order, lane j its joint, the frame's sums in joint order (every lane the same).
// PULL: the conditional pull of a visit is added after the pull towards the start, in the same way
template <bool JAC, bool PULL = false>
__device__ __forceinline__ SkelCost skel_eval(const SkelArgs& A, SkelLds& L, int c, long f, int g, int mask, double x0, double y0, double z0,
                                              const SkelPull q = {}) {
  const int lane = threadIdx.x, J = A.J;
  __syncthreads();
  if (lane == 0) {
    L.p[c][0][0] = L.r[c][0]; L.p[c][0][1] = L.r[c][1]; L.p[c][0][2] = L.r[c][2];
#pragma unroll 1
    for (int j = 1; j < J; ++j) {
      const int par = A.parent[j];
      const double len = L.len[j - 1];
      L.p[c][j][0] = L.p[c][par][0] + len * L.d[c][j - 1][0];
      L.p[c][j][1] = L.p[c][par][1] + len * L.d[c][j - 1][1];
      L.p[c][j][2] = L.p[c][par][2] + len * L.d[c][j - 1][2];
    }
  }
  __syncthreads();
  bool deep = true;
  if (lane < J) {
    const int j = lane;
    const double x = L.p[c][j][0], y = L.p[c][j][1], z = L.p[c][j][2];
    LiftGN e = lift_gn_start();
#pragma unroll
    for (int v = 0; v < SK_MAXV; ++v) {
      if (!((mask >> v) & 1)) continue;                                 // (mask holds no bit at or above V)
      const long gv = (long)g * A.V + v;
      const long o = ((long)v * A.Ftot + f) * A.J + j;
      Rot3 R;
      lift_rot3(A.quat + gv * 4, R);
      const LiftCam K = lift_cam(A.intr + gv * 9);
      const float* T = A.trans + gv * 3;
      const double w = A.kp_weight != nullptr ? (double)A.kp_weight[o] : 1.0;
      const double wx = x - (double)T[0], wy = y - (double)T[1], wz = z - (double)T[2];
      const double X = R.r00 * wx + R.r10 * wy + R.r20 * wz, Y = R.r01 * wx + R.r11 * wy + R.r21 * wz, Z = R.r02 * wx + R.r12 * wy + R.r22 * wz;
      if (!(Z > 0.0)) e.deep = false;
      const LiftProj pr = lift_project<JAC>(X, Y, Z, A.kp + o * 2, K, A.distort);
      const double ee = pr.du * pr.du + pr.dv * pr.dv;
      const double t = 1.0 + ee / A.sigma2;                             // (sigma = +inf: exactly 1)
      e.W += w;
      e.E += w * sqrt(ee);
      e.F += w * (ee / t);
      if (JAC) {
        const double wt = w * (1.0 / (t * t));
        const double j00 = pr.c00 * R.r00 + pr.c01 * R.r01 + pr.c02 * R.r02, j01 = pr.c00 * R.r10 + pr.c01 * R.r11 + pr.c02 * R.r12,
                     j02 = pr.c00 * R.r20 + pr.c01 * R.r21 + pr.c02 * R.r22;                                // J_pi R^T: with respect to the world point
        const double j10 = pr.c10 * R.r00 + pr.c11 * R.r01 + pr.c12 * R.r02, j11 = pr.c10 * R.r10 + pr.c11 * R.r11 + pr.c12 * R.r12,
                     j12 = pr.c10 * R.r20 + pr.c11 * R.r21 + pr.c12 * R.r22;
        lift_normal3_add(e.n, wt, pr.du, pr.dv, j00, j01, j02, j10, j11, j12);
      }
    }
    if (A.prior > 0.0) {                                                // the pull towards the start
      const double dx = x - x0, dy = y - y0, dz = z - z0;
      e.F += A.prior * ((dx * dx + dy * dy) + dz * dz);
      if (JAC) {
        e.n.H00 += A.prior; e.n.H11 += A.prior; e.n.H22 += A.prior;
        e.n.g0 += A.prior * dx; e.n.g1 += A.prior * dy; e.n.g2 += A.prior * dz;
      }
    }
    if (PULL) {                                                         // the pull towards q_j: the smoothness terms with the neighbours fixed
      const double dx = x - q.x, dy = y - q.y, dz = z - q.z;
      e.F += q.lam * ((dx * dx + dy * dy) + dz * dz);
      if (JAC) {
        e.n.H00 += q.lam; e.n.H11 += q.lam; e.n.H22 += q.lam;
        e.n.g0 += q.lam * dx; e.n.g1 += q.lam * dy; e.n.g2 += q.lam * dz;
      }
    }
    deep = e.deep;
    L.Fj[j] = e.F; L.Ej[j] = e.E; L.Wj[j] = e.W;
    if (JAC) {
      L.S[j][0] = e.n.H00; L.S[j][1] = e.n.H01; L.S[j][2] = e.n.H02; L.S[j][3] = e.n.H11; L.S[j][4] = e.n.H12; L.S[j][5] = e.n.H22;
      L.g[j][0] = e.n.g0; L.g[j][1] = e.n.g1; L.g[j][2] = e.n.g2;
    }
  }
  __syncthreads();
  SkelCost out = {0.0, 0.0, 0.0, __all(deep) != 0};
#pragma unroll 1
  for (int j = 0; j < J; ++j) { out.F += L.Fj[j]; out.E += L.Ej[j]; out.W += L.Wj[j]; }
  return out;
}

// 4. to 8. of the rule: from slot s's state and the sums skel_eval left, the candidate into slot c; false: no step
__device__ __forceinline__ bool skel_step(const SkelArgs& A, SkelLds& L, int s, int c) {
  const int lane = threadIdx.x, J = A.J, NB = J - 1, U = 3 + 2 * NB;
  // 4. subtree sums from the leaves: lane e owns entry e of (S, g)
  if (lane < 9) {
#pragma unroll 1
    for (int j = J - 1; j >= 1; --j) {
      const int par = A.parent[j];
      if (lane < 6) L.S[par][lane] += L.S[j][lane]; else L.g[par][lane - 6] += L.g[j][lane - 6];
    }
  }
  __syncthreads();
  // 5. lane b: the tangent basis of bone b, B = len [e1 e2], M = T_{b+1} B
  if (lane < NB) {
    const int b = lane;
    const double d0 = L.d[s][b][0], d1 = L.d[s][b][1], d2 = L.d[s][b][2], len = L.len[b];
    const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
    const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);     // the axis where |d| is smallest, the lowest on a tie
    const double dk = k == 0 ? d0 : (k == 1 ? d1 : d2);
    const double u0 = (k == 0 ? 1.0 : 0.0) - dk * d0, u1 = (k == 1 ? 1.0 : 0.0) - dk * d1, u2 = (k == 2 ? 1.0 : 0.0) - dk * d2;
    const double n = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
    const double e10 = u0 / n, e11 = u1 / n, e12 = u2 / n;
    const double e20 = d1 * e12 - d2 * e11, e21 = d2 * e10 - d0 * e12, e22 = d0 * e11 - d1 * e10;
    L.e1[b][0] = e10; L.e1[b][1] = e11; L.e1[b][2] = e12;
    L.e2[b][0] = e20; L.e2[b][1] = e21; L.e2[b][2] = e22;
    const double B00 = len * e10, B01 = len * e20, B10 = len * e11, B11 = len * e21, B20 = len * e12, B21 = len * e22;
    L.B[b][0] = B00; L.B[b][1] = B01; L.B[b][2] = B10; L.B[b][3] = B11; L.B[b][4] = B20; L.B[b][5] = B21;
    const double* T = L.S[b + 1];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double t0 = sk_sym(T, i, 0), t1 = sk_sym(T, i, 1), t2 = sk_sym(T, i, 2);
      L.M[b][2 * i] = (t0 * B00 + t1 * B10) + t2 * B20;
      L.M[b][2 * i + 1] = (t0 * B01 + t1 * B11) + t2 * B21;
    }
  }
  __syncthreads();
  // 6. the system: the last lane the root's block, lane b the two rows of bone b
  if (lane == SK_THREADS - 1) {
    const double* T = L.S[0];
    L.H[0] = T[0]; L.H[1] = T[1]; L.H[2] = T[3]; L.H[3] = T[2]; L.H[4] = T[4]; L.H[5] = T[5];
    L.rhs[0] = L.g[0][0]; L.rhs[1] = L.g[0][1]; L.rhs[2] = L.g[0][2];
  }
  if (lane < NB) {
    const int b = lane;
    const unsigned anc = A.anc[b];
    const double* Mb = L.M[b];
#pragma unroll 1
    for (int cb = 0; cb < 2; ++cb) {
      const int row = 3 + 2 * b + cb;
      double* Hrow = L.H + sk_idx(row, 0);
      Hrow[0] = Mb[cb]; Hrow[1] = Mb[2 + cb]; Hrow[2] = Mb[4 + cb];
#pragma unroll 1
      for (int a = 0; a <= b; ++a) {
        const bool on = (anc >> a) & 1u;
        const double* Ba = L.B[a];
        for (int ca = 0; ca < 2; ++ca) {
          const int col = 3 + 2 * a + ca;
          if (col > row) continue;
          Hrow[col] = on ? (Ba[ca] * Mb[cb] + Ba[2 + ca] * Mb[2 + cb]) + Ba[4 + ca] * Mb[4 + cb] : 0.0;
        }
      }
      const double* Bb = L.B[b];
      const double* h = L.g[b + 1];
      L.rhs[row] = (Bb[cb] * h[0] + Bb[2 + cb] * h[1]) + Bb[4 + cb] * h[2];
    }
  }
  __syncthreads();
  // 7. the factor, column by column: every lane the pivot (the same bits), the lanes stride over the column's rows
#pragma unroll 1
  for (int k = 0; k < U; ++k) {
    const double* Hk = L.H + sk_idx(k, 0);
    const double hkk = Hk[k];
    double a = hkk;
#pragma unroll 1
    for (int m = 0; m < k; ++m) a -= Hk[m] * Hk[m];
    if (!(__builtin_isfinite(a) && a > SK_PIVOT * hkk)) return false;   // (every lane alike)
    const double lkk = sqrt(a);
    if (lane == 0) L.diag[k] = lkk;
#pragma unroll 1
    for (int i = k + 1 + lane; i < U; i += SK_THREADS) {
      double* Hi = L.H + sk_idx(i, 0);
      double v = Hi[k];
#pragma unroll 1
      for (int m = 0; m < k; ++m) v -= Hi[m] * Hk[m];
      Hi[k] = v / lkk;
    }
    __syncthreads();
  }
  // forward and back substitution in index order: lane 0
  if (lane == 0) {
#pragma unroll 1
    for (int i = 0; i < U; ++i) {
      const double* Hi = L.H + sk_idx(i, 0);
      double v = L.rhs[i];
#pragma unroll 1
      for (int k = 0; k < i; ++k) v -= Hi[k] * L.x[k];
      L.x[i] = v / L.diag[i];
    }
#pragma unroll 1
    for (int i = U - 1; i >= 0; --i) {
      double v = L.x[i];
#pragma unroll 1
      for (int k = i + 1; k < U; ++k) v -= L.H[sk_idx(k, i)] * L.x[k];
      L.x[i] = v / L.diag[i];
    }
  }
  __syncthreads();
  // 8. the candidate
  bool finite = true;
  if (lane < 3) {
    const double v = L.r[s][lane] - L.x[lane];
    L.r[c][lane] = v;
    finite = __builtin_isfinite(v);
  }
  if (lane >= 3 && lane - 3 < NB) {                                     // (3 + 31 lanes at most)
    const int b = lane - 3;
    const double da = L.x[3 + 2 * b], db = L.x[4 + 2 * b];
    const double t0 = (L.d[s][b][0] - da * L.e1[b][0]) - db * L.e2[b][0], t1 = (L.d[s][b][1] - da * L.e1[b][1]) - db * L.e2[b][1],
                 t2 = (L.d[s][b][2] - da * L.e1[b][2]) - db * L.e2[b][2];
    const double n = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
    const double n0 = t0 / n, n1 = t1 / n, n2 = t2 / n;
    L.d[c][b][0] = n0; L.d[c][b][1] = n1; L.d[c][b][2] = n2;
    finite = __builtin_isfinite(n0) && __builtin_isfinite(n1) && __builtin_isfinite(n2);
  }
  return __all(finite) != 0;                                            // (skel_eval opens with a barrier)
}

// 2. the observations of lane j's joint: bit v of the mask.  For the visit kernel; lift_fit_skeleton_kernel keeps the same lines in place, where the
// compiler schedules them as it did before this header existed (through this function mp_lift_fit_skeleton's kernel comes out re-scheduled)
__device__ __forceinline__ int skel_observed(const SkelArgs& A, long f, int g) {
  const int lane = threadIdx.x, J = A.J;
  int mask = 0;
  if (lane < J) {
#pragma unroll
    for (int v = 0; v < SK_MAXV; ++v) {
      if (v >= A.V || !lift_view_ok(A.valid, A.quat, A.V, A.Ftot, f, g, v)) continue;      // an invalid view's data is never looked at
      const long o = ((long)v * A.Ftot + f) * J + lane;
      const double ku = A.kp[o * 2], kv = A.kp[o * 2 + 1];
      const double w = A.kp_weight != nullptr ? (double)A.kp_weight[o] : 1.0;
      if (__builtin_isfinite(ku) && __builtin_isfinite(kv) && __builtin_isfinite(w) && w > 0.0) mask |= 1 << v;
    }
  }
  return mask;
}

// slot s of the LDS state into a frame's 6 J doubles, or back: r, then the directions, then the positions
template <bool STORE>
__device__ __forceinline__ void skel_state(SkelLds& L, int s, double* st, int J) {
  const int lane = threadIdx.x, NB = J - 1;
  for (int i = lane; i < 3 + 3 * NB + 3 * J; i += SK_THREADS) {
    double* at = i < 3 ? &L.r[s][i] : (i < 3 + 3 * NB ? &L.d[s][(i - 3) / 3][(i - 3) % 3] : &L.p[s][(i - 3 - 3 * NB) / 3][(i - 3 - 3 * NB) % 3]);
    if (STORE) st[i] = *at; else *at = st[i];
  }
}

// rules 0 to 10 for the frame of this workgroup.  JAC = false: the launch of iters = 0, which takes no step and needs no Jacobian (F, E, W and
// deep have the same bits either way).  STATE: mp_lift_fit_skeleton_smooth's stage A, which also keeps the state in fp64, writes err as
// (Ftot, 3) with the result's E / W twice, and clears moves
template <bool JAC, bool STATE = false>
__global__ __launch_bounds__(SK_THREADS) void lift_fit_skeleton_kernel(SkelArgs A) {
  __shared__ SkelLds L;
  const long f = blockIdx.x;
  const int lane = threadIdx.x, J = A.J, NB = J - 1;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  if (f < fr.f0 || f >= fr.f1) return;                                  // a frame no take holds is left unwritten
  // 0. is the frame fitted at all
  double x0 = 0.0, y0 = 0.0, z0 = 0.0;
  bool fine = A.start_ok == nullptr || A.start_ok[f] != 0;
  if (lane < J) {
    const float* P = A.start + (f * J + lane) * 3;
    x0 = P[0]; y0 = P[1]; z0 = P[2];
    fine = fine && __builtin_isfinite(x0) && __builtin_isfinite(y0) && __builtin_isfinite(z0);
  }
  if (lane < NB) {
    const double len = A.lengths[(long)g * NB + lane];
    L.len[lane] = len;
    fine = fine && __builtin_isfinite(len) && len > 0.0;
  }
  unsigned char okbits = 0, taken = 0;
  double err0 = 0.0, err1 = 0.0;
  int s = -1;                                                           // the slot of the state; -1: no result
  if (__all(fine)) {
    // 1. the start: the root, the bones' directions
    if (lane == 0) { L.r[0][0] = x0; L.r[0][1] = y0; L.r[0][2] = z0; }
    if (lane >= 1 && lane < J) {
      const float* Q = A.start + (f * J + A.parent[lane]) * 3;
      const double vx = x0 - (double)Q[0], vy = y0 - (double)Q[1], vz = z0 - (double)Q[2];
      const double n = sqrt((vx * vx + vy * vy) + vz * vz);
      const bool own = __builtin_isfinite(n) && n > SK_DIR;
      L.own[lane - 1] = own;
      if (own) { L.d[0][lane - 1][0] = vx / n; L.d[0][lane - 1][1] = vy / n; L.d[0][lane - 1][2] = vz / n; }
    }
    __syncthreads();
    bool all_own = true;
    if (lane == 0) {
#pragma unroll 1
      for (int b = 0; b < NB; ++b) {
        if (L.own[b]) continue;
        all_own = false;
        const int par = A.parent[b + 1];                                // the direction of the parent's bone, (0, 0, 1) under the root
        L.d[0][b][0] = par > 0 ? L.d[0][par - 1][0] : 0.0;
        L.d[0][b][1] = par > 0 ? L.d[0][par - 1][1] : 0.0;
        L.d[0][b][2] = par > 0 ? L.d[0][par - 1][2] : 1.0;
      }
    }
    okbits = __all(all_own) ? 2 : 0;
    // 2. the observations of lane j's joint
    int mask = 0;
    if (lane < J) {
#pragma unroll
      for (int v = 0; v < SK_MAXV; ++v) {
        if (v >= A.V || !lift_view_ok(A.valid, A.quat, A.V, A.Ftot, f, g, v)) continue;    // an invalid view's data is never looked at
        const long o = ((long)v * A.Ftot + f) * J + lane;
        const double ku = A.kp[o * 2], kv = A.kp[o * 2 + 1];
        const double w = A.kp_weight != nullptr ? (double)A.kp_weight[o] : 1.0;
        if (__builtin_isfinite(ku) && __builtin_isfinite(kv) && __builtin_isfinite(w) && w > 0.0) mask |= 1 << v;
      }
    }
    const bool seen = __any(mask != 0) != 0;
    // 3. to 9. one loop: the start, then the steps
    LiftGN e = lift_gn_start();
    int c = 0;
#pragma unroll 1
    for (;;) {
      const SkelCost k = skel_eval<JAC>(A, L, c, f, g, mask, x0, y0, z0);
      LiftGN n = lift_gn_start();
      n.F = k.F; n.E = k.E; n.W = k.W; n.deep = k.deep;
      if (s < 0) {
        if (!(n.deep && __builtin_isfinite(n.F))) break;
        err0 = seen ? n.E / n.W : 0.0;
      } else {
        if (!lift_gn_accept(n, e)) break;
        ++taken;
      }
      s = c; c = 1 - s; e = n;
      if (!JAC || (int)taken >= A.iters) break;
      if (!skel_step(A, L, s, c)) break;
    }
    if (s >= 0) {
      okbits |= 1;
      err1 = seen ? e.E / e.W : 0.0;
    } else {
      err0 = 0.0;
    }
  }
  // 10.
  __syncthreads();
  float* out = A.pose + f * J * 3;
  for (int i = lane; i < J * 3; i += SK_THREADS) out[i] = s >= 0 ? (float)L.p[s][i / 3][i % 3] : 0.f;
  if (STATE && s >= 0) skel_state<true>(L, s, A.state + f * (6 * J), J);
  if (lane == 0) {
    constexpr int NE = STATE ? 3 : 2;
    A.err[f * NE] = (float)err0; A.err[f * NE + 1] = (float)err1;
    if (STATE) A.err[f * NE + 2] = (float)err1;
    A.ok[f] = okbits;
    if (A.steps != nullptr) A.steps[f] = taken;
    if (STATE && A.moves != nullptr) A.moves[f] = 0;
  }
}

// host: the checks of mp_lift_fit_skeleton's arguments under the caller's name, and the kernel's arguments
static int skel_arguments(const char* who, const float* start, const uint8_t* start_ok, const float* kp, const float* kp_weight, int V, int64_t Ftot,
                          int J, const uint8_t* valid, const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr,
                          const float* lengths, const int32_t* parents, int distort, float sigma, float prior, int iters, float* pose, float* err,
                          uint8_t* ok, uint8_t* steps, SkelArgs& a) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(start && kp && take_offset && quat && trans && intr && lengths, MP_ERR_ARG, "%s: null input", who);
  MP_CHECK(pose && err && ok, MP_ERR_ARG, "%s: null output", who);
  if (int rc = lift_take_shape(who, V, (long)Ftot, J, G)) return rc;
  MP_CHECK(distort == 0 || distort == 1, MP_ERR_ARG, "%s: distort=%d (0: project_to_2d_linear, 1: project_to_2d)", who, distort);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_REFINE_MAXITERS, MP_ERR_ARG, "%s: iters=%d outside 0..%d", who, iters, MP_LIFT_REFINE_MAXITERS);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "%s: sigma=%g must be > 0 (inf: every robust factor is 1)", who, (double)sigma);
  MP_CHECK(prior >= 0.f && __builtin_isfinite(prior), MP_ERR_ARG, "%s: prior=%g must be finite and >= 0", who, (double)prior);
  MP_CHECK((long)Ftot <= 0x7fffffffL, MP_ERR_ARG, "%s: %ld frames: too many for one launch", who, (long)Ftot);
  a = {};
  if (int rc = rigid_parents(who, parents, J, a.parent)) return rc;
  for (int b = 0; b < J - 1; ++b) a.anc[b] = (1u << b) | (a.parent[b + 1] > 0 ? a.anc[a.parent[b + 1] - 1] : 0u);
  a.start = start; a.start_ok = start_ok; a.kp = kp; a.kp_weight = kp_weight; a.valid = valid; a.take_offset = (const long*)take_offset;
  a.quat = quat; a.trans = trans; a.intr = intr; a.lengths = lengths; a.pose = pose; a.err = err; a.ok = ok; a.steps = steps;
  a.Ftot = (long)Ftot; a.sigma2 = (double)sigma * (double)sigma; a.prior = (double)prior;
  a.V = V; a.J = J; a.G = G; a.distort = distort; a.iters = iters;
  return MP_OK;
}

}  // namespace mp
