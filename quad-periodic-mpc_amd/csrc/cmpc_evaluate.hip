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
#include "cmpc_rigid64.h"

namespace cmpc {
namespace {

struct EvalShared {
  double scr[kEvS0];
  double st[12 * (MAXN + 1)];  // d_k, then 2 W e_k, then lambda_k+1; slot N: the input of U = 0
  double ts[6 * MAXN];         // t, s of phase A; y, nu/m of phase D
  float u[12 * MAXN];
  float traj[12 * MAXN];
};

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
    rigid_setup(rec, ib0, ib1, ib2, scr);
  }
  wsync();

  // ---- A: per step and axis, sum_f (r_f x u_f)_a and sum_f u_f,a over all four feet
  foot_sums(lane, N, rec, sh.u, sh.ts);
  wsync();

  // ---- B: d_k,j = (Bdt u_k + Qdt f)_j + (Adt's column of the gravity state) x0[12]; slot k = N: U = 0
  {
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
      const double c = step_input(j, tq, sq, scr[19], grav, scr, dt, dth, dt3, im64);
      sh.st[t] = c;
    }
  }
  wsync();

  // ---- C: lane j < 12 owns component j of x (and of the U = 0 trajectory), then of lambda
  double cacc = 0.0, c0acc = 0.0;
  {
    const int jj = (lane < 12) ? lane : 11;
    float wf = 0.f;
#pragma unroll
    for (int i = 0; i < 12; i++) wf = (jj == i) ? P.wts[i] : wf;
    const double wj = (double)wf;
    // x_j += (N1 x)_j + d_k,j  (N1 = Adt - I: rows 0..2 dt R' x[6:9]; 3, 4 dt x9, x10;
    // 5 dt x11 + dt^2/2 x_drag x9; 11 dt x_drag x9; the gravity state's terms are in d)
    const N1Row n1 = n1_row(jj, scr, dt, dth);
    const double c6 = n1.c6, c7 = n1.c7, c8 = n1.c8, c9 = n1.c9, c10 = n1.c10, c11 = n1.c11;
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
    const N1tRow n1t = n1t_row(jj, scr, dt, dth);
    const double e0c = n1t.e0, e1c = n1t.e1, e2c = n1t.e2, e3c = n1t.e3, e4c = n1t.e4, e5c = n1t.e5, e11c = n1t.e11;
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
