// cmpc_evaluate.hip — cmpc_batch_evaluate: for given forces U (12N per instance, any source), the
// predicted trajectory, the tracking cost and a rigorous optimality gap of the exact QP the fp32
// record defines, all in fp64 and without forming H, g, Adt or Bdt (include/cmpc_solver.h states
// the formulas). One wavefront per instance (one single-wave workgroup each, so no s_barrier), the
// instance's data staged in LDS.
//
// A_c^3 = 0 (ct_ss_mats, SolverMPC.cpp:260-279), so with N1 = dt A_c + dt^2/2 A_c^2
//   Adt = I + N1,  Bdt = (dt I + dt^2/2 A_c + dt^3/6 A_c^2) B_c,  Qdt likewise with Q_c
// exactly, and both act as a few sparse operations (the arithmetic of refine_residual's phases
// A-D, cmpc_wide.h, over all 12N columns instead of a reduced variable list):
//   0  forces and traj into LDS; R, I_world^-1 (fp64 from the fp32 quaternion) and x_0
//   A  lane (k, a): t_a = sum_f (r_f x u_kf)_a and s_a = sum_f u_kf,a of step k
//   B  lane (k, j): the step input d_k,j = (Bdt u_k + Qdt f)_j + the gravity state's share; slot
//      k = N holds the input of U = 0 (for cost0)
//   C  lanes 0..11 own one state component: x_k+1 = Adt x_k + d_k with the cross terms by
//      v_readlane, the U = 0 trajectory beside it; then the adjoint lambda <- Adt' lambda + 2 W e_k
//   D  lane (k, i): y_k = I_world^-1 nu_k[6:9] and nu_k[9:12] / m, nu_k = (dt I + dt^2/2 A_c' +
//      dt^3/6 A_c'^2) lambda_k+1
//   E  lane (k, f): the gradient of foot-step (k, f), (y_k x r_f) + nu_k[9:12]/m + 2 alpha u, and
//      its gap / slack / swing terms
//   F  xor-butterfly reductions over the wave: the same order for every instance, whatever the batch
#ifndef CMPC_EVALUATE_INST
#define CMPC_EVALUATE_INST 0  // 1: the per-instance build (a second unit of this file; see the kernel below)
#endif
#include "cmpc_common.h"

namespace cmpc {
namespace {

constexpr int kEvS0 = 32;  // scr: [0..8] R, [9..17] I_world^-1, [18] x_drag, [19] f_est(3) term, [20..31] x_0

struct EvalShared {
  double scr[kEvS0];
  double st[12 * (MAXN + 1)];  // d_k, then 2 W e_k, then lambda_k+1; slot N: the input of U = 0
  double ts[6 * MAXN];         // t, s of phase A; y, nu/m of phase D
  float u[12 * MAXN];
  float traj[12 * MAXN];
};

// x_0's rpy exactly as the reference pipeline's restatement evaluates quat_to_rpy
// (SolverMPC.cpp:352-361): the arguments in fp32 with every product and sum rounded (no fused
// multiply-add), the inverse trigonometric functions in fp64, the result rounded to fp32.
__device__ __forceinline__ void rpy_rounded(const float* __restrict__ rec, double* rpy) {
  const float w = rec[CMPC_REC_Q + 0], x = rec[CMPC_REC_Q + 1], y = rec[CMPC_REC_Q + 2], z = rec[CMPC_REC_Q + 3];
  const float ww = __fmul_rn(w, w), xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), zz = __fmul_rn(z, z);
  double asd = -2.0 * (double)__fsub_rn(__fmul_rn(x, z), __fmul_rn(w, y));
  if (!(asd < .99999)) asd = .99999;  // only the upper clamp, as the reference
  const float as = (float)asd;
  const float n0 = __fmul_rn(2.f, __fadd_rn(__fmul_rn(y, z), __fmul_rn(w, x)));
  const float d0 = __fadd_rn(__fsub_rn(__fsub_rn(ww, xx), yy), zz);
  const float n2 = __fmul_rn(2.f, __fadd_rn(__fmul_rn(x, y), __fmul_rn(w, z)));
  const float d2 = __fsub_rn(__fsub_rn(__fadd_rn(ww, xx), yy), zz);
  rpy[0] = (double)(float)atan2((double)n0, (double)d0);
  rpy[1] = (double)(float)asin((double)as);
  rpy[2] = (double)(float)atan2((double)n2, (double)d2);
}

// NaN-propagating maximum (fmax drops a NaN operand; non-finite input is to show in the result)
__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ double bfly_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double bfly_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = nmax(v, __shfl_xor(v, m, 64));
  return v;
}

// CMPC_EVALUATE_INST = 1 (this file's second unit in build.py's UNITS): the per-instance build
// for a handle with a table (cmpc_batch_set_instance_params, _set_instance_costs), a kernel and a launcher of their own
// names in a unit of their own, so that this unit compiles the shared kernel exactly as before. The
// kernel's body is the one below: instance i first takes its inertia doubles from row i of the
// handle's snapshot of the rows and 1 / m, 1 / mu, f_max, the weights and alpha from its table entry.
#if CMPC_EVALUATE_INST
__global__ __launch_bounds__(64) void cmpc_evaluate_inst_kernel(const float* __restrict__ d_recs,
                                                                const float* __restrict__ d_forces, int batch,
                                                                KParams P, double alpha,
                                                                const double* __restrict__ inst_rows,
                                                                float* __restrict__ d_xpred,
                                                                double* __restrict__ d_cert) {
  __shared__ EvalShared sh;
  const int inst = blockIdx.x;
  if (inst >= batch) return;
  const double* row = inst_rows + (size_t)inst * CMPC_INST_WORDS;
  const double ib0 = row[CMPC_INST_INERTIA], ib1 = row[CMPC_INST_INERTIA + 1], ib2 = row[CMPC_INST_INERTIA + 2];
  {
    const KInst* e = P.inst + inst;
    P.mdl.im64 = e->mdl.im64;
    P.mu_inv = e->mu_inv;
    P.f_max = e->f_max;
    // (the cost by scalar loads, the instance being the workgroup's: the weights stay uniform
    // values, as the shared kernel's are)
    const KInst* eu = inst_entry(P, inst);
    float w[13];
    cost_weights<true>(P, eu, w);
#pragma unroll
    for (int j = 0; j < 12; j++) P.wts[j] = w[j];
    P.alpha2 = inst_late<float>(eu, kInstAlpha2Off);
    alpha = inst_late<double>(eu, (int)offsetof(KInst, alpha64));
  }
#else
__global__ __launch_bounds__(64) void cmpc_evaluate_kernel(const float* __restrict__ d_recs,
                                                           const float* __restrict__ d_forces, int batch,
                                                           KParams P, double alpha, double ib0,
                                                           double ib1, double ib2,
                                                           float* __restrict__ d_xpred,
                                                           double* __restrict__ d_cert) {
  __shared__ EvalShared sh;
  const int inst = blockIdx.x;
  if (inst >= batch) return;
#endif
  const int lane = threadIdx.x;
  const int N = P.N;
  const float* __restrict__ rec = d_recs + (size_t)inst * P.rec_words;
  const float* __restrict__ uin = d_forces + (size_t)inst * 12 * N;
  const double dt = P.dt64, dth = P.dth64, dt3 = P.dt3_64;
  const double im64 = P.mdl.im64;  // 1 / m of the handle's model
  double* scr = sh.scr;

  // ---- 0: forces and traj into LDS (sum of u^2 on the way), the instance's matrices and x_0
  double usq = 0.0;
  for (int c = lane; c < 12 * N; c += 64) {
    const float uv = uin[c];
    sh.u[c] = uv;
    sh.traj[c] = rec[CMPC_REC_HDR + c];
    usq += (double)uv * (double)uv;
  }
  if (lane == 0) {
    // R (Eigen toRotationMatrix, RobotState.cpp:36) and I_world = R I_body R' (SolverMPC.cpp:593;
    // I_body = diag(ib0, ib1, ib2), the handle's model; RobotState.h:25 is the default) in fp64
    // from the fp32 quaternion; the inverse by cofactors
    const double qw = rec[CMPC_REC_Q + 0], qx = rec[CMPC_REC_Q + 1], qy = rec[CMPC_REC_Q + 2],
                 qz = rec[CMPC_REC_Q + 3];
    double R[9];
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz); R[1] = 2.0 * (qx * qy - qw * qz); R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz); R[4] = 1.0 - 2.0 * (qx * qx + qz * qz); R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy); R[7] = 2.0 * (qy * qz + qw * qx); R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    double Iw[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++)
        Iw[3 * i + j] = R[3 * i] * ib0 * R[3 * j] + R[3 * i + 1] * ib1 * R[3 * j + 1] +
                        R[3 * i + 2] * ib2 * R[3 * j + 2];
    const double c00 = Iw[4] * Iw[8] - Iw[5] * Iw[7];
    const double c10 = Iw[5] * Iw[6] - Iw[3] * Iw[8];
    const double c20 = Iw[3] * Iw[7] - Iw[4] * Iw[6];
    const double idet = 1.0 / (Iw[0] * c00 + Iw[1] * c10 + Iw[2] * c20);
#pragma unroll
    for (int i = 0; i < 9; i++) scr[i] = R[i];
    scr[9] = c00 * idet;  scr[10] = (Iw[2] * Iw[7] - Iw[1] * Iw[8]) * idet; scr[11] = (Iw[1] * Iw[5] - Iw[2] * Iw[4]) * idet;
    scr[12] = c10 * idet; scr[13] = (Iw[0] * Iw[8] - Iw[2] * Iw[6]) * idet; scr[14] = (Iw[2] * Iw[3] - Iw[0] * Iw[5]) * idet;
    scr[15] = c20 * idet; scr[16] = (Iw[1] * Iw[6] - Iw[0] * Iw[7]) * idet; scr[17] = (Iw[0] * Iw[4] - Iw[1] * Iw[3]) * idet;
    const uint32_t flags = __float_as_uint(rec[CMPC_REC_FLAGS]);
    scr[18] = (double)rec[CMPC_REC_XDRAG];
    scr[19] = (flags & 1u) ? (double)rec[CMPC_REC_FEST3] : 0.0;  // Q_c f (SolverMPC.cpp:808-811)
    rpy_rounded(rec, &scr[20]);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      scr[23 + i] = (double)rec[CMPC_REC_P + i];
      scr[26 + i] = (double)rec[CMPC_REC_W + i];
      scr[29 + i] = (double)rec[CMPC_REC_V + i];
    }
  }
  wsync();

  // ---- A: per step and axis, sum_f (r_f x u_f)_a and sum_f u_f,a over all four feet
  if (lane < 3 * N) {
    const int k = lane / 3, a = lane - 3 * k;
    const int a1 = (a == 2) ? 0 : a + 1, a2 = (a == 0) ? 2 : a - 1;
    double tc = 0.0, sc = 0.0;
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const float* uf = &sh.u[12 * k + 3 * f];
      // (r x u)_a = r_a1 u_a2 - r_a2 u_a1
      tc += (double)rec[CMPC_REC_R + 4 * a1 + f] * (double)uf[a2] - (double)rec[CMPC_REC_R + 4 * a2 + f] * (double)uf[a1];
      sc += (double)uf[a];
    }
    sh.ts[6 * k + a] = tc;
    sh.ts[6 * k + 3 + a] = sc;
  }
  wsync();

  // ---- B: d_k,j = (Bdt u_k + Qdt f)_j + (Adt's column of the gravity state) x0[12]; slot k = N: U = 0
  {
    const double* R = scr;
    const double* Ii = scr + 9;
    const double xd = scr[18];
    const double grav = (double)(-9.8f);  // x0[12] (SolverMPC.cpp:592)
    for (int t = lane; t < 12 * (N + 1); t += 64) {
      const int k = t / 12, j = t - 12 * k;
      const bool zero = (k == N);
      const double* tsk = &sh.ts[6 * (zero ? 0 : k)];
      double tq[3], sq[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        tq[i] = zero ? 0.0 : tsk[i];
        sq[i] = zero ? 0.0 : tsk[3 + i];
      }
      // w = B_c u_k + Q_c f: w[6:9] = I_world^-1 t, w[9:12] = s / m (+ f_est(3) into row 9)
      const double w9 = sq[0] * im64 + scr[19];
      double c;
      if (j < 3 || (j >= 6 && j < 9)) {
        c = 0.0;
#pragma unroll
        for (int m = 0; m < 3; m++) {
          const double wm = Ii[3 * m] * tq[0] + Ii[3 * m + 1] * tq[1] + Ii[3 * m + 2] * tq[2];
          c += (j < 3) ? dth * R[3 * m + j] * wm : ((j - 6 == m) ? dt * wm : 0.0);
        }
      } else if (j == 3 || j == 9) {
        c = ((j == 3) ? dth : dt) * w9;
      } else if (j == 4 || j == 10) {
        c = ((j == 4) ? dth : dt) * sq[1] * im64;
      } else if (j == 5) {
        c = dth * sq[2] * im64 + dt3 * xd * w9 + dth * grav;
      } else {
        c = dt * sq[2] * im64 + dth * xd * w9 + dt * grav;
      }
      sh.st[t] = c;
    }
  }
  wsync();

  // ---- C: lane j < 12 owns component j of x (and of the U = 0 trajectory), then of lambda
  double cacc = 0.0, c0acc = 0.0;
  {
    const int jj = (lane < 12) ? lane : 11;
    const double* R = scr;
    float wf = 0.f;
#pragma unroll
    for (int i = 0; i < 12; i++) wf = (jj == i) ? P.wts[i] : wf;
    const double wj = (double)wf;
    // x_j += (N1 x)_j + d_k,j  (N1 = Adt - I: rows 0..2 dt R' x[6:9]; 3, 4 dt x9, x10;
    // 5 dt x11 + dt^2/2 x_drag x9; 11 dt x_drag x9; the gravity state's terms are in d)
    double c6 = 0.0, c7 = 0.0, c8 = 0.0, c9 = 0.0, c10 = 0.0, c11 = 0.0;
    if (jj < 3) { c6 = dt * R[jj]; c7 = dt * R[3 + jj]; c8 = dt * R[6 + jj]; }
    if (jj == 3) c9 = dt;
    if (jj == 4) c10 = dt;
    if (jj == 5) { c11 = dt; c9 = dth * scr[18]; }
    if (jj == 11) c9 = dt * scr[18];
    double x = scr[20 + jj], x0 = x;
    const double d0 = sh.st[12 * N + jj];
    float* xp = d_xpred ? d_xpred + (size_t)inst * 12 * N : nullptr;
    for (int k = 0; k < N; k++) {
      const double dk = sh.st[12 * k + jj];
      const double xdes = (double)sh.traj[12 * k + jj];
      const double z6 = rl_d(x, 6), z7 = rl_d(x, 7), z8 = rl_d(x, 8);
      const double z9 = rl_d(x, 9), z10 = rl_d(x, 10), z11 = rl_d(x, 11);
      x += c6 * z6 + c7 * z7 + c8 * z8 + c9 * z9 + c10 * z10 + c11 * z11 + dk;
      const double y6 = rl_d(x0, 6), y7 = rl_d(x0, 7), y8 = rl_d(x0, 8);
      const double y9 = rl_d(x0, 9), y10 = rl_d(x0, 10), y11 = rl_d(x0, 11);
      x0 += c6 * y6 + c7 * y7 + c8 * y8 + c9 * y9 + c10 * y10 + c11 * y11 + d0;
      const double e = x - xdes, e0 = x0 - xdes;
      cacc += wj * e * e;
      c0acc += wj * e0 * e0;
      if (lane < 12) {
        sh.st[12 * k + lane] = 2.0 * wj * e;  // 2 W e_k+1
        if (xp) xp[12 * k + lane] = (float)x;
      }
    }
    if (lane >= 12) { cacc = 0.0; c0acc = 0.0; }
    // lambda_j += (N1' lambda)_j + 2 W e  (rows 6..8 dt R lambda[0:3]; 9 dt (l3 + x_drag l11) +
    // dt^2/2 x_drag l5; 10 dt l4; 11 dt l5)
    double lam = 0.0;
    double e0c = 0.0, e1c = 0.0, e2c = 0.0, e3c = 0.0, e4c = 0.0, e5c = 0.0, e11c = 0.0;
    if (jj >= 6 && jj < 9) { e0c = dt * R[3 * (jj - 6)]; e1c = dt * R[3 * (jj - 6) + 1]; e2c = dt * R[3 * (jj - 6) + 2]; }
    if (jj == 9) { e3c = dt; e11c = dt * scr[18]; e5c = dth * scr[18]; }
    if (jj == 10) e4c = dt;
    if (jj == 11) e5c = dt;
    for (int k = N - 1; k >= 0; k--) {
      const double sk = sh.st[12 * k + jj];
      const double m0 = rl_d(lam, 0), m1 = rl_d(lam, 1), m2 = rl_d(lam, 2), m3 = rl_d(lam, 3);
      const double m4 = rl_d(lam, 4), m5 = rl_d(lam, 5), m11 = rl_d(lam, 11);
      lam += e0c * m0 + e1c * m1 + e2c * m2 + e3c * m3 + e4c * m4 + e5c * m5 + e11c * m11 + sk;
      if (lane < 12) sh.st[12 * k + lane] = lam;
    }
  }
  wsync();

  // ---- D: per step, y_k = I_world^-1 nu_k[6:9] (i < 3) and nu_k[9 + i - 3] / m into ts
  for (int t = lane; t < 6 * N; t += 64) {
    const int k = t / 6, i = t - 6 * k;
    const double* lm = &sh.st[12 * k];
    const double* R = scr;
    const double* Ii = scr + 9;
    const double xd = scr[18];
    double ev = 0.0;
    if (i < 3) {
#pragma unroll
      for (int m = 0; m < 3; m++) {
        const double nu = dt * lm[6 + m] + dth * (R[3 * m] * lm[0] + R[3 * m + 1] * lm[1] + R[3 * m + 2] * lm[2]);
        ev += Ii[3 * i + m] * nu;
      }
    } else if (i == 3) {
      ev = (dt * lm[9] + dth * (lm[3] + xd * lm[11]) + dt3 * xd * lm[5]) * im64;
    } else if (i == 4) {
      ev = (dt * lm[10] + dth * lm[4]) * im64;
    } else {
      ev = (dt * lm[11] + dth * lm[5]) * im64;
    }
    sh.ts[t] = ev;
  }
  wsync();

  // ---- E: foot-step (k, f): gradient, gap term, slack, swing force
  double gap = 0.0, viol = 0.0, swing = 0.0, gmax = 0.0;
  {
    const double mu_inv = (double)P.mu_inv;  // 1/mu as fmat holds it in fp32 (SolverMPC.cpp:657)
    const double mu = 1.0 / mu_inv;
    const double nrm = 1.0 / sqrt(mu_inv * mu_inv + 1.0);
    const unsigned char* gait = reinterpret_cast<const unsigned char*>(rec + CMPC_REC_GAIT(N));
    for (int t = lane; t < 4 * N; t += 64) {
      const int k = t >> 2, f = t & 3;
      const double* yp = &sh.ts[6 * k];
      const double r0 = (double)rec[CMPC_REC_R + f], r1 = (double)rec[CMPC_REC_R + 4 + f],
                   r2 = (double)rec[CMPC_REC_R + 8 + f];
      const double u0 = (double)sh.u[3 * t], u1 = (double)sh.u[3 * t + 1], u2 = (double)sh.u[3 * t + 2];
      // ub(fz) = gait x f_max in fp32; the foot-step is eliminated (swing) iff |ub| < 0.01
      // (SolverMPC.cpp:869-894, the test of every solver kernel)
      const float ubf = (float)gait[t] * P.f_max;
      if (ubf < 0.01f && ubf > -0.01f) {
        swing = nmax(swing, nmax(fabs(u0), nmax(fabs(u1), fabs(u2))));
      } else {
        const double ub = (double)ubf;
        const double g0 = yp[1] * r2 - yp[2] * r1 + yp[3] + 2.0 * alpha * u0;
        const double g1 = yp[2] * r0 - yp[0] * r2 + yp[4] + 2.0 * alpha * u1;
        const double g2 = yp[0] * r1 - yp[1] * r0 + yp[5] + 2.0 * alpha * u2;
        // Frank-Wolfe gap of the truncated pyramid: vertices 0 and (+-mu ub, +-mu ub, ub)
        const double vmin = ub * (g2 - mu * fabs(g0) - mu * fabs(g1));
        gap += (g0 * u0 + g1 * u1 + g2 * u2) - ((vmin < 0.0) ? vmin : 0.0);
        gmax = nmax(gmax, nmax(fabs(g0), nmax(fabs(g1), fabs(g2))));
        // negative slack of the six rows, the friction rows normalised to unit length
        double s = nmax(-u2, u2 - ub);
        s = nmax(s, -(u0 * mu_inv + u2) * nrm);
        s = nmax(s, -(-u0 * mu_inv + u2) * nrm);
        s = nmax(s, -(u1 * mu_inv + u2) * nrm);
        s = nmax(s, -(-u1 * mu_inv + u2) * nrm);
        viol = nmax(viol, s);
      }
    }
  }

  // ---- F: wave reductions (xor butterfly: one fixed order), lane 0 writes the certificate
  const double cost_t = bfly_sum(cacc);
  const double cost_0 = bfly_sum(c0acc);
  const double usum = bfly_sum(usq);
  gap = bfly_sum(gap);
  viol = bfly_max(viol);
  swing = bfly_max(swing);
  gmax = bfly_max(gmax);
  if (d_cert && lane == 0) {
    double* o = d_cert + (size_t)inst * CMPC_CERT_WORDS;
    o[CMPC_CERT_COST] = cost_t + alpha * usum;
    o[CMPC_CERT_COST0] = cost_0;
    o[CMPC_CERT_GAP] = gap;
    o[CMPC_CERT_VIOL] = viol;
    o[CMPC_CERT_SWING] = swing;
    o[CMPC_CERT_GRADMAX] = gmax;
    o[6] = 0.0;
    o[7] = 0.0;
  }
}

}  // namespace

#if CMPC_EVALUATE_INST
hipError_t launch_evaluate_inst(const float* d_recs, const float* d_forces, int batch, const KParams& P,
                                double alpha, const double* inst_rows, float* d_xpred, double* d_cert,
                                hipStream_t stream) {
  hipLaunchKernelGGL(cmpc_evaluate_inst_kernel, dim3(batch), dim3(64), 0, stream, d_recs, d_forces, batch, P,
                     alpha, inst_rows, d_xpred, d_cert);
  return hipGetLastError();
}
#else
hipError_t launch_evaluate_inst(const float* d_recs, const float* d_forces, int batch, const KParams& P,
                                double alpha, const double* inst_rows, float* d_xpred, double* d_cert,
                                hipStream_t stream);  // this file's CMPC_EVALUATE_INST unit

hipError_t launch_evaluate(const float* d_recs, const float* d_forces, int batch, const KParams& P,
                           double alpha, const double* ib64, float* d_xpred, double* d_cert,
                           hipStream_t stream, const double* inst_rows) {
  if (batch <= 0) return hipSuccess;
  if (P.inst)
    return inst_rows ? launch_evaluate_inst(d_recs, d_forces, batch, P, alpha, inst_rows, d_xpred, d_cert, stream)
                     : hipErrorInvalidValue;
  hipLaunchKernelGGL(cmpc_evaluate_kernel, dim3(batch), dim3(64), 0, stream, d_recs, d_forces, batch, P,
                     alpha, ib64[0], ib64[1], ib64[2], d_xpred, d_cert);
  return hipGetLastError();
}
#endif

}  // namespace cmpc
