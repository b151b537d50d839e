// cmpc_gain.hip — cmpc_batch_gain: the step-0 feedback gain G = d u_0* / d x_0 of the minimiser over
// the face of the friction pyramids that given forces U lie on, by the backward half of
// cmpc_sensitivity.hip's fp64 Riccati recursion (include/cmpc_solver.h states the quantity, DESIGN.md
// §15 the layout and what was measured); and cmpc_batch_feedback, which applies it. One wavefront per
// instance (one single-wave workgroup each, so no s_barrier), static LDS only. The model's closed
// forms are cmpc_rigid64.h's, the face and the columns of Z_k cmpc_face.h's.
//
// With Pn = P_k+1 + W kept in LDS (P_N = 0), G_k = Bdt Z_k (d = d_k columns) and Adt = I + N1 applied
// by N1's non-zeros (n1_col: at most three per column), per step k = N-1 .. 0:
//   S1  G = Bdt Z_k [12][d];  PA = Pn + Pn N1                     48 lanes, three entries of one column each
//   S2  T = G'Pn [d][12]                                          12 d entries, 12 products each
//   S3  R = alpha Z_k'Z_k + T G [d][d]
//   S4  lane i < d takes row i of R, lane c < 12 column c of M = T + T N1 (= G'Pn Adt), in registers;
//       Cholesky R = L L' right-looking and Y = L^-1 M, the other operand broadcast by v_readlane
//   S5  P_k = PA + N1'PA - Y'Y, + W on the diagonal: the next step's Pn
// At k = 0 S4 goes on to K_0 = L^-T Y and G = -Z_0 K_0, and the recursion ends; PA and S5 are not
// needed there. Every sum runs in one order whatever the batch or the instance's place in it.
#ifndef CMPC_GAIN_INST
#define CMPC_GAIN_INST 0  // 1: the per-instance build (a second unit of this file, as cmpc_sensitivity.hip's)
#endif
#include "cmpc_face.h"

namespace cmpc {
namespace {

struct GainShared {
  double scr[kEvS0];       // rigid_frame's part of it: R, I_world^-1, x_drag
  double B[144];           // Bdt over the 12 dynamic states, row-major
  double Pn[144], PA[144]; // P_k+1 + W; Pn Adt (before the recursion PA holds the staged forces, fp32)
  double G[144], T[144];   // Bdt Z_k [12][column]; G'Pn [column][12], then Y [column][12]
  double Rm[144];          // R [column][column], stride 12
  double W[12];
  float zv[36 * MAXN];     // column c of step k: its three coefficients at 3 (12 k + c), exact in fp32
  unsigned char zf[12 * MAXN];  // column c of step k: its foot
  unsigned char dk[MAXN];       // columns of step k
};
static_assert(sizeof(float) * 12 * MAXN <= sizeof(double) * 144, "the staged forces fit in PA");

// Phase profiler (diagnostic builds of this unit only, -DCMPC_GAIN_PHASE_PROF; scripts/gain_phase_prof.py):
// lane 0 of every instance adds the clock64() cycles of each phase to g_gain_phase. 0 set-up (staging,
// frame, Bdt, the face), 1..3 S1..S3, 4 S4 (with Y's store), 5 S5, 6 step 0's back substitution and G
#ifdef CMPC_GAIN_PHASE_PROF
__device__ unsigned long long g_gain_phase[8];
#define GP_MARK(i)                                                      \
  do {                                                                  \
    const unsigned long long _n = clock64();                            \
    if (lane == 0) atomicAdd(&g_gain_phase[i], _n - t_last);            \
    t_last = _n;                                                        \
  } while (0)
#else
#define GP_MARK(i) do {} while (0)
#endif

// lane c < 12 writes column c of G (acc: its twelve rows), lane 0 the words after it
__device__ __forceinline__ void gain_store(double* __restrict__ o, int lane, const double (&acc)[12], double poison,
                                           double mfree, int d0, double smin) {
  if (lane < 12) {
#pragma unroll
    for (int row = 0; row < 12; row++) o[CMPC_GAIN_K + 12 * row + lane] = acc[row] + poison;
  }
  if (lane == 0) {
    o[CMPC_GAIN_FREE] = mfree;
    o[CMPC_GAIN_FREE0] = (double)d0;
    o[CMPC_GAIN_SLACK] = smin + poison;
    o[147] = 0.0;
  }
}

#if CMPC_GAIN_INST
__global__ __launch_bounds__(64) void cmpc_gain_inst_kernel(
    const float* __restrict__ d_recs, const float* __restrict__ d_forces, int batch, KParams P, double alpha,
    const double* __restrict__ inst_rows, double act_tol, double* __restrict__ d_gain) {
  __shared__ GainShared sh;
  const int inst = blockIdx.x;
  if (inst >= batch) return;
  const double* row = inst_rows + (size_t)inst * CMPC_INST_WORDS;
  const double ib0 = row[CMPC_INST_INERTIA], ib1 = row[CMPC_INST_INERTIA + 1], ib2 = row[CMPC_INST_INERTIA + 2];
  {
    // instance i's 1 / m, 1 / mu, f_max, weights and alpha from its table entry, as
    // cmpc_sensitivity_inst_kernel takes them
    const KInst* e = P.inst + inst;
    P.mdl.im64 = e->mdl.im64;
    P.mu_inv = e->mu_inv;
    P.f_max = e->f_max;
    const KInst* eu = inst_entry(P, inst);
    float w[13];
    cost_weights<true>(P, eu, w);
#pragma unroll
    for (int j = 0; j < 12; j++) P.wts[j] = w[j];
    alpha = inst_late<double>(eu, (int)offsetof(KInst, alpha64));
  }
#else
__global__ __launch_bounds__(64) void cmpc_gain_kernel(
    const float* __restrict__ d_recs, const float* __restrict__ d_forces, int batch, KParams P, double alpha,
    double ib0, double ib1, double ib2, double act_tol, double* __restrict__ d_gain) {
  __shared__ GainShared sh;
  const int inst = blockIdx.x;
  if (inst >= batch) return;
#endif
  const int lane = threadIdx.x;
  const int N = P.N;
  const float* __restrict__ rec = d_recs + (size_t)inst * P.rec_words;
  const float* __restrict__ uin = d_forces + (size_t)inst * 12 * N;
  const double dt = P.dt64, dth = P.dth64, dt3 = P.dt3_64;
  const double im64 = P.mdl.im64;
  double* scr = sh.scr;
#ifdef CMPC_GAIN_PHASE_PROF
  unsigned long long t_last = clock64();
#endif

  // ---- 0: the forces into LDS; `poison` is 0, or NaN when one of them is not finite
  float* us = reinterpret_cast<float*>(sh.PA);
  double poison = 0.0;
  for (int c = lane; c < 12 * N; c += 64) {
    const float uv = uin[c];
    us[c] = uv;
    poison += 0.0 * (double)uv;
  }
  if (lane == 0) rigid_frame(rec, ib0, ib1, ib2, scr);
  if (lane < 12) {
    float wf = 0.f;
#pragma unroll
    for (int i = 0; i < 12; i++) wf = (lane == i) ? P.wts[i] : wf;
    sh.W[lane] = (double)wf;
  }
  wsync();

  // ---- A: Bdt dense (column 3 f + a: the unit force e_a on foot f), Pn = W; lane k classifies step
  // k's foot-steps and lists the columns of Z_k
  for (int e = lane; e < 144; e += 64) {
    const int i = e / 12, c = e - 12 * i;
    const int f = c / 3, ax = c - 3 * f;
    double tq[3], sq[3];
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const int b1 = (b == 2) ? 0 : b + 1, b2 = (b == 0) ? 2 : b - 1;
      // (r x e_ax)_b = r_b1 [ax == b2] - r_b2 [ax == b1]
      tq[b] = ((ax == b2) ? (double)rec[CMPC_REC_R + 4 * b1 + f] : 0.0) -
              ((ax == b1) ? (double)rec[CMPC_REC_R + 4 * b2 + f] : 0.0);
      sq[b] = (ax == b) ? 1.0 : 0.0;
    }
    sh.B[e] = step_input(i, tq, sq, 0.0, 0.0, scr, dt, dth, dt3, im64);
    sh.Pn[e] = (i == c) ? sh.W[i] : 0.0;
  }
  double mfree = 0.0, smin = __builtin_inf();
  if (lane < N) {
    const int col = face_columns(lane, N, rec, us, P, act_tol, &sh.zf[12 * lane], &sh.zv[36 * lane], smin);
    sh.dk[lane] = (unsigned char)col;
    mfree = (double)col;
  }
  poison = bfly_sum(poison);
  mfree = bfly_sum(mfree);
  smin = bfly_min(smin);
  // the entries of a 12 x 12 matrix that lane l < 48 owns: column lc = l % 12 of the rows l / 12 + 4 r,
  // r = 0..2 (one column per lane, so N1's column lc serves X N1 in every round and the lane's column of
  // M in S4; N1's column i serves N1'X)
  const int lc = lane % 12, lq = (lane < 48) ? lane / 12 : 3;
  const N1Col nc = n1_col(lc, scr, dt, dth);
  N1Col ni[3];
  double wd[3];  // W_i where the entry is on the diagonal, else 0
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const int i = lq + 4 * r;
    ni[r] = n1_col(i, scr, dt, dth);
    wd[r] = (i == lc) ? sh.W[i] : 0.0;
  }
  const int lr = (lane < 12) ? lane : 11;
  wsync();
  GP_MARK(0);

  // ---- the backward recursion
  double* o = d_gain + (size_t)inst * CMPC_GAIN_WORDS;
  for (int k = N - 1; k >= 0; k--) {
    const int d = __builtin_amdgcn_readfirstlane((int)sh.dk[k]);
    const float* zv = &sh.zv[36 * k];
    const unsigned char* zf = &sh.zf[12 * k];
    if (k == 0 && d == 0) {  // nothing free at step 0: G = 0
      double acc[12];
#pragma unroll
      for (int j = 0; j < 12; j++) acc[j] = 0.0;
      gain_store(o, lane, acc, poison, mfree, 0, smin);
      break;
    }
    // S1
    if (lane < 48) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const int i = lq + 4 * r, c = lc, e = 12 * i + c;
        if (c < d) {
          const int f = zf[c];
          sh.G[e] = sh.B[12 * i + 3 * f] * (double)zv[3 * c] + sh.B[12 * i + 3 * f + 1] * (double)zv[3 * c + 1] +
                    sh.B[12 * i + 3 * f + 2] * (double)zv[3 * c + 2];
        }
        if (k > 0) {
          const double* Pi = &sh.Pn[12 * i];
          double s = Pi[c];
          s += Pi[nc.r0] * nc.v0;
          s += Pi[nc.r1] * nc.v1;
          s += Pi[nc.r2] * nc.v2;
          sh.PA[e] = s;
        }
      }
    }
    wsync();
    GP_MARK(1);
    // S2
    for (int e = lane; e < 12 * d; e += 64) {
      const int j = e / 12, c = e - 12 * j;
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 12; r++) s += sh.G[12 * r + j] * sh.Pn[12 * r + c];
      sh.T[e] = s;
    }
    wsync();
    GP_MARK(2);
    // S3 (Z_k'Z_k is block diagonal over the feet)
    for (int e = lane; e < 12 * d; e += 64) {
      const int j = e / 12, c = e - 12 * j;
      if (c < d) {
        double s = (zf[j] == zf[c]) ? alpha * ((double)zv[3 * j] * (double)zv[3 * c] +
                                               (double)zv[3 * j + 1] * (double)zv[3 * c + 1] +
                                               (double)zv[3 * j + 2] * (double)zv[3 * c + 2])
                                    : 0.0;
#pragma unroll
        for (int r = 0; r < 12; r++) s += sh.T[12 * j + r] * sh.G[12 * r + c];
        sh.Rm[e] = s;
      }
    }
    wsync();
    GP_MARK(3);
    // S4: a = row `lane` of R, then of L with 1 / L[j][j] on the diagonal (lanes >= d hold zeros);
    // m = column lc of M, then of Y
    double a[12], m[12];
#pragma unroll
    for (int t = 0; t < 12; t++) {
      a[t] = 0.0;
      m[t] = 0.0;
      if (t < d) {
        const double rv = sh.Rm[12 * lr + t];
        a[t] = (lane < d) ? rv : 0.0;
        const double* Tj = &sh.T[12 * t];
        double s = Tj[lc];
        s += Tj[nc.r0] * nc.v0;
        s += Tj[nc.r1] * nc.v1;
        s += Tj[nc.r2] * nc.v2;
        m[t] = s;
      }
    }
    wsync();  // T is read: Y may take its place
#pragma unroll
    for (int j = 0; j < 12; j++) {
      if (j < d) {
        const double piv = rl_d(a[j], j);
        const double iv = 1.0 / sqrt(piv);
        const double l = a[j] * iv;  // L[lane][j]
        a[j] = (lane == j) ? iv : l;  // the diagonal holds 1 / L[j][j]
#pragma unroll
        for (int t = j + 1; t < 12; t++)
          if (t < d) a[t] -= l * rl_d(l, t);
      }
    }
#pragma unroll
    for (int j = 0; j < 12; j++) {
      if (j < d) {
        double s = m[j];
#pragma unroll
        for (int t = 0; t < j; t++) s -= rl_d(a[t], j) * m[t];
        m[j] = s * rl_d(a[j], j);
      }
    }
    if (k == 0) {
      GP_MARK(4);
      // K_0 = L^-T Y in place, then column lc of G = -Z_0 K_0: an axis of a foot sums its columns in
      // their order; a foot without a column keeps +0.0
#pragma unroll
      for (int i = 11; i >= 0; i--) {
        if (i < d) {
          double s = m[i];
#pragma unroll
          for (int t = i + 1; t < 12; t++)
            if (t < d) s -= rl_d(a[i], t) * m[t];
          m[i] = s * rl_d(a[i], i);
        }
      }
      double acc[12];
#pragma unroll
      for (int j = 0; j < 12; j++) acc[j] = 0.0;
#pragma unroll
      for (int j = 0; j < 12; j++) {
        if (j < d) {
          const int f = __builtin_amdgcn_readfirstlane((int)zf[j]);
          const double z0 = (double)zv[3 * j], z1 = (double)zv[3 * j + 1], z2 = (double)zv[3 * j + 2];
#pragma unroll
          for (int ff = 0; ff < 4; ff++) {
            if (f == ff) {
              acc[3 * ff] -= z0 * m[j];
              acc[3 * ff + 1] -= z1 * m[j];
              acc[3 * ff + 2] -= z2 * m[j];
            }
          }
        }
      }
      gain_store(o, lane, acc, poison, mfree, d, smin);
      GP_MARK(6);
      break;
    }
    if (lane < 12) {
#pragma unroll
      for (int j = 0; j < 12; j++)
        if (j < d) sh.T[12 * j + lane] = m[j];
    }
    wsync();
    GP_MARK(4);
    // S5
    if (lane < 48) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const int i = lq + 4 * r, c = lc, e = 12 * i + c;
        double s = sh.PA[e];
        s += ni[r].v0 * sh.PA[12 * ni[r].r0 + c];
        s += ni[r].v1 * sh.PA[12 * ni[r].r1 + c];
        s += ni[r].v2 * sh.PA[12 * ni[r].r2 + c];
        for (int j = 0; j < d; j++) s -= sh.T[12 * j + i] * sh.T[12 * j + c];
        sh.Pn[e] = s + wd[r];
      }
    }
    wsync();
    GP_MARK(5);
  }
}

#if !CMPC_GAIN_INST
// cmpc_batch_feedback: 16 lanes per instance, lane r < 12 owns force component r of step 0 and row r
// of G (96 contiguous bytes as six 16-byte loads, so d_gain is 16-byte aligned; the instance's 1152 bytes
// of G are read whole, its four trailing words not). The group's first read is its
// due byte; a due instance touches nothing else.
constexpr int kFbLanes = 16, kFbBlock = 256;
__global__ __launch_bounds__(kFbBlock) void cmpc_feedback_kernel(
    const float* __restrict__ d_recs, const float* __restrict__ d_forces, const double* __restrict__ d_gain,
    const float* __restrict__ d_states, const uint8_t* __restrict__ d_due, int batch, KParams P,
    float* __restrict__ d_u) {
  const int inst = blockIdx.x * (kFbBlock / kFbLanes) + (int)(threadIdx.x / kFbLanes);
  const int l = threadIdx.x & (kFbLanes - 1);
  if (inst >= batch) return;
  if (d_due && d_due[inst] != 0) return;
  const int r = (l < 12) ? l : 11;
  const float* __restrict__ rec = d_recs + (size_t)inst * P.rec_words;
  float mu_inv = P.mu_inv, f_max = P.f_max;
  if (P.inst) {
    mu_inv = P.inst[inst].mu_inv;
    f_max = P.inst[inst].f_max;
  }
  const double2* __restrict__ g2 =
      reinterpret_cast<const double2*>(d_gain + (size_t)inst * CMPC_GAIN_WORDS + CMPC_GAIN_K + 12 * r);
  double g[12];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const double2 v = g2[c];
    g[2 * c] = v.x;
    g[2 * c + 1] = v.y;
  }
  // delta = x - x_0, x_0 as the solve forms it (rpy of the quaternion, rounded to fp32); the rpy
  // differences wrapped into [-pi, pi]
  double rpy[3];
  rpy_rounded(rec, rpy);
  const double x0 = (r < 3) ? ((r == 0) ? rpy[0] : (r == 1) ? rpy[1] : rpy[2])
                    : (r < 6) ? (double)rec[CMPC_REC_P + r - 3]
                    : (r < 9) ? (double)rec[CMPC_REC_W + r - 6]
                              : (double)rec[CMPC_REC_V + r - 9];
  double dl = (double)d_states[(size_t)inst * 12 + r] - x0;
  const double two_pi = 6.283185307179586;
  if (r < 3) dl = dl - two_pi * rint(dl / two_pi);
  double u = (double)d_forces[(size_t)inst * P.out_cols + r];
#pragma unroll
  for (int c = 0; c < 12; c++) u += g[c] * __shfl(dl, c, kFbLanes);
  // the guard, per foot of step 0
  const int f = r / 3, ax = r - 3 * f;
  const unsigned char* gait = reinterpret_cast<const unsigned char*>(rec + CMPC_REC_GAIT(P.N));
  const float ubf = (float)gait[f] * f_max;
  double fz = __shfl(u, 3 * f + 2, kFbLanes);
  fz = (fz > 0.0) ? fz : 0.0;
  fz = (fz < (double)ubf) ? fz : (double)ubf;
  const double lim = (1.0 / (double)mu_inv) * fz;
  double out = (u > -lim) ? u : -lim;
  out = (out < lim) ? out : lim;
  if (ax == 2) out = fz;
  if (ubf < 0.01f && ubf > -0.01f) out = 0.0;  // swing
  if (l < 12) d_u[(size_t)inst * 12 + l] = (float)out;
}
#endif

}  // namespace

#if CMPC_GAIN_INST
hipError_t launch_gain_inst(const float* d_recs, const float* d_forces, int batch, const KParams& P, double alpha,
                            const double* inst_rows, double act_tol, double* d_gain, hipStream_t stream) {
  hipLaunchKernelGGL(cmpc_gain_inst_kernel, dim3(batch), dim3(64), 0, stream, d_recs, d_forces, batch, P, alpha,
                     inst_rows, act_tol, d_gain);
  return hipGetLastError();
}
#else
hipError_t launch_gain_inst(const float* d_recs, const float* d_forces, int batch, const KParams& P, double alpha,
                            const double* inst_rows, double act_tol, double* d_gain,
                            hipStream_t stream);  // this file's CMPC_GAIN_INST unit

hipError_t launch_gain(const float* d_recs, const float* d_forces, int batch, const KParams& P, double alpha,
                       const double* ib64, double act_tol, double* d_gain, hipStream_t stream,
                       const double* inst_rows) {
  if (batch <= 0) return hipSuccess;
  if (P.inst)
    return inst_rows ? launch_gain_inst(d_recs, d_forces, batch, P, alpha, inst_rows, act_tol, d_gain, stream)
                     : hipErrorInvalidValue;
  hipLaunchKernelGGL(cmpc_gain_kernel, dim3(batch), dim3(64), 0, stream, d_recs, d_forces, batch, P, alpha,
                     ib64[0], ib64[1], ib64[2], act_tol, d_gain);
  return hipGetLastError();
}

#ifdef CMPC_GAIN_PHASE_PROF
// the phase counters (cycles summed over the instances since the last reset) -> out[8]; reset != 0 zeroes them
extern "C" int cmpc_gain_phase_read(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gain_phase), sizeof(g_gain_phase)) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_gain_phase), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

hipError_t launch_feedback(const float* d_recs, const float* d_forces, const double* d_gain, const float* d_states,
                           const uint8_t* d_due, int batch, const KParams& P, float* d_u, hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  const int per = kFbBlock / kFbLanes;
  hipLaunchKernelGGL(cmpc_feedback_kernel, dim3((batch + per - 1) / per), dim3(kFbBlock), 0, stream, d_recs,
                     d_forces, d_gain, d_states, d_due, batch, P, d_u);
  return hipGetLastError();
}
#endif

}  // namespace cmpc
