// cmpc_sensitivity.hip — cmpc_batch_sensitivity: for given forces U and an upstream gradient
// V = dL/dU, the gradients of L through the minimiser over the face of the friction pyramids that U
// lies on, by an fp64 Riccati adjoint (include/cmpc_solver.h states the quantity, DESIGN.md §14 the
// derivation). One wavefront per instance (one single-wave workgroup each, so no s_barrier), the
// instance's data staged in LDS as cmpc_evaluate.hip stages it; the model's closed forms are that
// kernel's (cmpc_rigid64.h).
//
// The adjoint w = -Z (Z'HZ)^-1 Z'V minimises sum_k dx_k+1' W dx_k+1 + alpha |w_k|^2 + V_k'w_k over
// w_k = Z_k y_k, dx_k+1 = Adt dx_k + Bdt w_k, dx_0 = 0: an LQ problem over the 12 dynamic states.
//   0  forces, V and traj into LDS; R, I_world^-1 and x_0; Adt and Bdt dense (12 x 12 each)
//   A  the step inputs d_k (evaluate's phases A, B), then x_k(U) - xd_k per step (its phase C)
//   B  lane k: the face of step k's four foot-steps, a closed-form basis per foot-step, the columns
//      of Z_k (at most 12) listed as (foot, three coefficients): face_columns, cmpc_face.h
//   C  backwards over the steps, with Pn = P_k+1 + W and G = Bdt Z_k:
//        R = alpha Z_k'Z_k + G'Pn G,  Cholesky,  K_k = R^-1 G'Pn Adt,  kappa_k = R^-1 (G'p_k+1 + Z_k'V_k / 2)
//        P_k = Adt'Pn Adt - (Adt'Pn G) K_k,  p_k = Adt'p_k+1 - (Adt'Pn G) kappa_k
//      the gains of all steps kept in LDS (the dynamic part: 156 doubles per step)
//   D  forwards: y_k = -K_k dx_k - kappa_k, w_k = Z_k y_k, dx_k+1 = Adt dx_k + Bdt w_k
//   E  lambda <- Adt'lambda + 2 W dx_k backwards (lanes 0..11 own a component, cross terms by
//      v_readlane), the per-lane products, xor-butterfly reductions: one order whatever the batch
#ifndef CMPC_SENSITIVITY_INST
#define CMPC_SENSITIVITY_INST 0  // 1: the per-instance build (a second unit of this file, as cmpc_evaluate.hip's)
#endif
#include "cmpc_face.h"

namespace cmpc {
namespace {

constexpr int kGain = 156;  // doubles per step of the gains: K_k [12 columns of Z_k][12], kappa_k [12]

struct SensShared {
  double scr[kEvS0];
  double A[144], B[144];        // Adt, Bdt over the 12 dynamic states, row-major
  double P[144], PA[144];       // P_k+1 (without W); Pn Adt
  double G[144], PG[144];       // Bdt Z_k, Pn G  [12][column]
  double M[144], Rm[144];       // G'Pn Adt [column][12]; R, then its Cholesky factor (lower)
  double p[2][12], q[12], y[12], wk[12], dx[2][12], W[12];
  double ld[12];                // the diagonal of the Cholesky factor
  double st[12 * MAXN];         // d_k, then x_k+1(U) - xd_k, then 2 W dx_k+1
  double ts[6 * MAXN];
  double zv[36 * MAXN];         // column c of step k: its three coefficients at 3 (12 k + c)
  float u[12 * MAXN], v[12 * MAXN], traj[12 * MAXN];
  unsigned char zf[12 * MAXN];  // column c of step k: its foot
  unsigned char dk[MAXN];       // columns of step k
};

#if CMPC_SENSITIVITY_INST
__global__ __launch_bounds__(64) void cmpc_sensitivity_inst_kernel(
    const float* __restrict__ d_recs, const float* __restrict__ d_forces, const float* __restrict__ d_gradf,
    int batch, KParams P, double alpha, const double* __restrict__ inst_rows, double act_tol,
    double* __restrict__ d_sens, double* __restrict__ d_dtraj, double* __restrict__ d_dg) {
  __shared__ SensShared sh;
  extern __shared__ double gains[];
  const int inst = blockIdx.x;
  if (inst >= batch) return;
  const double* row = inst_rows + (size_t)inst * CMPC_INST_WORDS;
  const double ib0 = row[CMPC_INST_INERTIA], ib1 = row[CMPC_INST_INERTIA + 1], ib2 = row[CMPC_INST_INERTIA + 2];
  {
    // instance i's 1 / m, 1 / mu, f_max, weights and alpha from its table entry, as
    // cmpc_evaluate_inst_kernel takes them
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
__global__ __launch_bounds__(64) void cmpc_sensitivity_kernel(
    const float* __restrict__ d_recs, const float* __restrict__ d_forces, const float* __restrict__ d_gradf,
    int batch, KParams P, double alpha, double ib0, double ib1, double ib2, double act_tol,
    double* __restrict__ d_sens, double* __restrict__ d_dtraj, double* __restrict__ d_dg) {
  __shared__ SensShared sh;
  extern __shared__ double gains[];
  const int inst = blockIdx.x;
  if (inst >= batch) return;
#endif
  const int lane = threadIdx.x;
  const int N = P.N;
  const float* __restrict__ rec = d_recs + (size_t)inst * P.rec_words;
  const float* __restrict__ uin = d_forces + (size_t)inst * 12 * N;
  const float* __restrict__ vin = d_gradf + (size_t)inst * 12 * N;
  const double dt = P.dt64, dth = P.dth64, dt3 = P.dt3_64;
  const double im64 = P.mdl.im64;
  double* scr = sh.scr;
  const int jj = (lane < 12) ? lane : 11;

  // ---- 0: forces, V and traj into LDS; `poison` is 0, or NaN when one of them is not finite
  double poison = 0.0;
  for (int c = lane; c < 12 * N; c += 64) {
    const float uv = uin[c], vv = vin[c], tv = rec[CMPC_REC_HDR + c];
    sh.u[c] = uv;
    sh.v[c] = vv;
    sh.traj[c] = tv;
    poison += 0.0 * (double)uv + 0.0 * (double)vv + 0.0 * (double)tv;
  }
  if (lane == 0) rigid_setup(rec, ib0, ib1, ib2, scr);
  if (lane < 12) {
    float wf = 0.f;
#pragma unroll
    for (int i = 0; i < 12; i++) wf = (lane == i) ? P.wts[i] : wf;
    sh.W[lane] = (double)wf;
  }
  wsync();

  // ---- A: the step inputs; Adt = I + N1 and Bdt dense (column 3 f + a of Bdt: the unit force e_a on foot f)
  foot_sums(lane, N, rec, sh.u, sh.ts);
  for (int e = lane; e < 144; e += 64) {
    const int i = e / 12, c = e - 12 * i;
    const N1Row n1 = n1_row(i, scr, dt, dth);
    double a = (i == c) ? 1.0 : 0.0;
    a += (c == 6) ? n1.c6 : (c == 7) ? n1.c7 : (c == 8) ? n1.c8 : (c == 9) ? n1.c9 : (c == 10) ? n1.c10
         : (c == 11) ? n1.c11 : 0.0;
    sh.A[e] = a;
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
  }
  wsync();
  {
    const double grav = (double)(-9.8f);  // x0[12] (SolverMPC.cpp:592)
    for (int t = lane; t < 12 * N; t += 64) {
      const int k = t / 12, j = t - 12 * k;
      double tq[3], sq[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        tq[i] = sh.ts[6 * k + i];
        sq[i] = sh.ts[6 * k + 3 + i];
      }
      sh.st[t] = step_input(j, tq, sq, scr[19], grav, scr, dt, dth, dt3, im64);
    }
  }
  wsync();
  // x_k+1 = Adt x_k + d_k as evaluate's phase C; st <- x_k+1(U) - xd_k (lane j < 12 owns component j)
  {
    const N1Row n1 = n1_row(jj, scr, dt, dth);
    double x = scr[20 + jj];
    for (int k = 0; k < N; k++) {
      const double dk = sh.st[12 * k + jj];
      const double xdes = (double)sh.traj[12 * k + jj];
      const double z6 = rl_d(x, 6), z7 = rl_d(x, 7), z8 = rl_d(x, 8);
      const double z9 = rl_d(x, 9), z10 = rl_d(x, 10), z11 = rl_d(x, 11);
      x += n1.c6 * z6 + n1.c7 * z7 + n1.c8 * z8 + n1.c9 * z9 + n1.c10 * z10 + n1.c11 * z11 + dk;
      if (lane < 12) sh.st[12 * k + lane] = x - xdes;
    }
  }

  // ---- B: lane k classifies step k's foot-steps and lists the columns of Z_k
  double mfree = 0.0, smin = __builtin_inf();
  if (lane < N) {
    const int k = lane;
    const int col = face_columns(k, N, rec, sh.u, P, act_tol, &sh.zf[12 * k], &sh.zv[36 * k], smin);
    sh.dk[k] = (unsigned char)col;
    mfree = (double)col;
  }
  for (int e = lane; e < 144; e += 64) sh.P[e] = 0.0;
  if (lane < 12) { sh.p[0][lane] = 0.0; sh.dx[0][lane] = 0.0; }
  wsync();

  // ---- C: the backward Riccati recursion
  int pb = 0;  // p_k+1 is sh.p[pb]
  for (int k = N - 1; k >= 0; k--) {
    const int d = __builtin_amdgcn_readfirstlane((int)sh.dk[k]);
    const double* zv = &sh.zv[36 * k];
    const unsigned char* zf = &sh.zf[12 * k];
    double* Kk = &gains[kGain * k];
    const double* pk = sh.p[pb];
    // C1: G = Bdt Z_k, PA = Pn Adt
    for (int e = lane; e < 144; e += 64) {
      const int i = e / 12, c = e - 12 * i;
      if (c < d) {
        const int f = zf[c];
        sh.G[e] = sh.B[12 * i + 3 * f] * zv[3 * c] + sh.B[12 * i + 3 * f + 1] * zv[3 * c + 1] +
                  sh.B[12 * i + 3 * f + 2] * zv[3 * c + 2];
      }
      double s = sh.W[i] * sh.A[e];
      for (int r = 0; r < 12; r++) s += sh.P[12 * i + r] * sh.A[12 * r + c];
      sh.PA[e] = s;
    }
    wsync();
    // C2: PG = Pn G, M = G'PA, q = G'p + Z_k'V_k / 2
    for (int e = lane; e < 144; e += 64) {
      const int i = e / 12, c = e - 12 * i;
      if (c < d) {
        double s = sh.W[i] * sh.G[e];
        for (int r = 0; r < 12; r++) s += sh.P[12 * i + r] * sh.G[12 * r + c];
        sh.PG[e] = s;
      }
      if (i < d) {  // M[i][c]: column i of Z_k, state c
        double s = 0.0;
        for (int r = 0; r < 12; r++) s += sh.G[12 * r + i] * sh.PA[12 * r + c];
        sh.M[e] = s;
      }
    }
    if (lane < d) {
      const float* vk = &sh.v[12 * k + 3 * zf[lane]];
      double s = 0.5 * (zv[3 * lane] * (double)vk[0] + zv[3 * lane + 1] * (double)vk[1] + zv[3 * lane + 2] * (double)vk[2]);
      for (int r = 0; r < 12; r++) s += sh.G[12 * r + lane] * pk[r];
      sh.q[lane] = s;
    }
    wsync();
    // C3: R = alpha Z_k'Z_k + G'PG (Z_k'Z_k is block diagonal over the feet)
    for (int e = lane; e < 144; e += 64) {
      const int i = e / 12, c = e - 12 * i;
      if (i < d && c < d) {
        double s = (zf[i] == zf[c])
                       ? alpha * (zv[3 * i] * zv[3 * c] + zv[3 * i + 1] * zv[3 * c + 1] + zv[3 * i + 2] * zv[3 * c + 2])
                       : 0.0;
        for (int r = 0; r < 12; r++) s += sh.G[12 * r + i] * sh.PG[12 * r + c];
        sh.Rm[e] = s;
      }
    }
    wsync();
    // C4: Cholesky R = L L', left-looking: lane i >= j finishes L[i][j] in round j (the diagonal's
    // sum recomputed by every lane, so one exchange per round; the diagonal itself goes to ld)
    for (int j = 0; j < d; j++) {
      if (lane >= j && lane < d) {
        double s = sh.Rm[12 * lane + j], sd = sh.Rm[12 * j + j];
        for (int t = 0; t < j; t++) {
          const double ljt = sh.Rm[12 * j + t];
          s -= sh.Rm[12 * lane + t] * ljt;
          sd -= ljt * ljt;
        }
        const double ljj = sqrt(sd);
        if (lane == j) sh.ld[j] = ljj;
        else sh.Rm[12 * lane + j] = s / ljj;
      }
      wsync();
    }
    // C5: K_k = R^-1 M (lane j < 12 owns column j), kappa_k = R^-1 q (lane 12), in place in the gains
    if (lane < 13 && d > 0) {
      const double* src = (lane < 12) ? &sh.M[lane] : sh.q;
      double* dst = (lane < 12) ? &Kk[lane] : &Kk[144];
      const int sst = (lane < 12) ? 12 : 1;
      for (int i = 0; i < d; i++) {
        double s = src[sst * i];
        for (int t = 0; t < i; t++) s -= sh.Rm[12 * i + t] * dst[sst * t];
        dst[sst * i] = s / sh.ld[i];
      }
      for (int i = d - 1; i >= 0; i--) {
        double s = dst[sst * i];
        for (int t = i + 1; t < d; t++) s -= sh.Rm[12 * t + i] * dst[sst * t];
        dst[sst * i] = s / sh.ld[i];
      }
    }
    wsync();
    // C6: P_k = Adt'PA - M'K_k, p_k = Adt'p_k+1 - M'kappa_k
    for (int e = lane; e < 144; e += 64) {
      const int i = e / 12, c = e - 12 * i;
      double s = 0.0;
      for (int r = 0; r < 12; r++) s += sh.A[12 * r + i] * sh.PA[12 * r + c];
      for (int r = 0; r < d; r++) s -= sh.M[12 * r + i] * Kk[12 * r + c];
      sh.P[e] = s;
    }
    if (lane < 12) {
      double s = 0.0;
      for (int r = 0; r < 12; r++) s += sh.A[12 * r + lane] * pk[r];
      for (int r = 0; r < d; r++) s -= sh.M[12 * r + lane] * Kk[144 + r];
      sh.p[pb ^ 1][lane] = s;
    }
    pb ^= 1;
    wsync();
  }

  // ---- D: forwards. Lane a < 12 owns force column a of the step, lane j < 12 state component j
  double wu = 0.0, wacc = 0.0;
  {
    double* dtr = d_dtraj ? d_dtraj + (size_t)inst * 12 * N : nullptr;
    double* dgo = d_dg ? d_dg + (size_t)inst * 12 * N : nullptr;
    const double wj = sh.W[jj];
    int xb = 0;
    for (int k = 0; k < N; k++) {
      const int d = __builtin_amdgcn_readfirstlane((int)sh.dk[k]);
      const double* zv = &sh.zv[36 * k];
      const unsigned char* zf = &sh.zf[12 * k];
      const double* Kk = &gains[kGain * k];
      const double* dx = sh.dx[xb];
      if (lane < d) {
        double s = -Kk[144 + lane];
        for (int r = 0; r < 12; r++) s -= Kk[12 * lane + r] * dx[r];
        sh.y[lane] = s;
      }
      wsync();
      if (lane < 12) {
        const int f = lane / 3, ax = lane - 3 * f;
        double s = 0.0;
        for (int c = 0; c < d; c++)
          if (zf[c] == f) s += zv[3 * c + ax] * sh.y[c];
        sh.wk[lane] = s;
        wu += s * (double)sh.u[12 * k + lane];
        if (dgo) dgo[12 * k + lane] = s;
      }
      wsync();
      if (lane < 12) {
        double s = 0.0;
        for (int r = 0; r < 12; r++) s += sh.A[12 * lane + r] * dx[r];
        for (int r = 0; r < 12; r++) s += sh.B[12 * lane + r] * sh.wk[r];
        sh.dx[xb ^ 1][lane] = s;
        wacc += s * sh.st[12 * k + lane];
        if (dtr) dtr[12 * k + lane] = -2.0 * wj * s;
        sh.st[12 * k + lane] = 2.0 * wj * s;
      }
      xb ^= 1;
      wsync();
    }
  }

  // ---- E: lambda_k = Adt'lambda_k+1 + 2 W dx_k (k = N .. 1), dL/df_est(3) = sum_k lambda_k'Qdt e_3,
  // dL/dx_0 = Adt'lambda_1; then the reductions
  double lam = 0.0, facc = 0.0;
  {
    const N1tRow n1t = n1t_row(jj, scr, dt, dth);
    const double zero3[3] = {0.0, 0.0, 0.0};
    const double q3 = step_input(jj, zero3, zero3, 1.0, 0.0, scr, dt, dth, dt3, im64);  // (Qdt e_3)_j
    for (int k = N - 1; k >= -1; k--) {
      const double sk = (k >= 0) ? sh.st[12 * k + jj] : 0.0;
      const double m0 = rl_d(lam, 0), m1 = rl_d(lam, 1), m2 = rl_d(lam, 2), m3 = rl_d(lam, 3);
      const double m4 = rl_d(lam, 4), m5 = rl_d(lam, 5), m11 = rl_d(lam, 11);
      lam += n1t.e0 * m0 + n1t.e1 * m1 + n1t.e2 * m2 + n1t.e3 * m3 + n1t.e4 * m4 + n1t.e5 * m5 + n1t.e11 * m11 + sk;
      if (k >= 0) facc += lam * q3;
    }
    if (lane >= 12) facc = 0.0;
  }
  poison = bfly_sum(poison);
  const double fsum = bfly_sum(facc);
  const double wusum = bfly_sum(wu);
  mfree = bfly_sum(mfree);
  smin = bfly_min(smin);
  double* o = d_sens + (size_t)inst * CMPC_SENS_WORDS;
  if (lane < 12) {
    o[CMPC_SENS_X0 + lane] = lam + poison;
    o[CMPC_SENS_WEIGHTS + lane] = 2.0 * wacc + poison;
  }
  if (lane == 0) {
    const uint32_t flags = __float_as_uint(rec[CMPC_REC_FLAGS]);
    o[CMPC_SENS_ALPHA] = 2.0 * wusum + poison;
    o[CMPC_SENS_FEST3] = ((flags & 1u) ? fsum : 0.0) + poison;
    o[CMPC_SENS_FREE] = mfree;
    o[CMPC_SENS_SLACK] = smin + poison;
    o[28] = 0.0;
    o[29] = 0.0;
    o[30] = 0.0;
    o[31] = 0.0;
  }
}

}  // namespace

#if CMPC_SENSITIVITY_INST
hipError_t launch_sensitivity_inst(const float* d_recs, const float* d_forces, const float* d_gradf, int batch,
                                   const KParams& P, double alpha, const double* inst_rows, double act_tol,
                                   double* d_sens, double* d_dtraj, double* d_dg, hipStream_t stream) {
  hipLaunchKernelGGL(cmpc_sensitivity_inst_kernel, dim3(batch), dim3(64), sizeof(double) * kGain * P.N, stream,
                     d_recs, d_forces, d_gradf, batch, P, alpha, inst_rows, act_tol, d_sens, d_dtraj, d_dg);
  return hipGetLastError();
}
#else
hipError_t launch_sensitivity_inst(const float* d_recs, const float* d_forces, const float* d_gradf, int batch,
                                   const KParams& P, double alpha, const double* inst_rows, double act_tol,
                                   double* d_sens, double* d_dtraj, double* d_dg,
                                   hipStream_t stream);  // this file's CMPC_SENSITIVITY_INST unit

hipError_t launch_sensitivity(const float* d_recs, const float* d_forces, const float* d_gradf, int batch,
                              const KParams& P, double alpha, const double* ib64, double act_tol, double* d_sens,
                              double* d_dtraj, double* d_dg, hipStream_t stream, const double* inst_rows) {
  if (batch <= 0) return hipSuccess;
  if (P.inst)
    return inst_rows ? launch_sensitivity_inst(d_recs, d_forces, d_gradf, batch, P, alpha, inst_rows, act_tol,
                                               d_sens, d_dtraj, d_dg, stream)
                     : hipErrorInvalidValue;
  hipLaunchKernelGGL(cmpc_sensitivity_kernel, dim3(batch), dim3(64), sizeof(double) * kGain * P.N, stream, d_recs,
                     d_forces, d_gradf, batch, P, alpha, ib64[0], ib64[1], ib64[2], act_tol, d_sens, d_dtraj, d_dg);
  return hipGetLastError();
}
#endif

}  // namespace cmpc
