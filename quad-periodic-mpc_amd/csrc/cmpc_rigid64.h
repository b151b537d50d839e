// cmpc_rigid64.h — what the fp64 kernels of one wavefront per instance share (cmpc_evaluate.hip,
// cmpc_sensitivity.hip, cmpc_gain.hip): the instance's matrices from the fp32 record, and the exact discretisation
// in closed form. A_c^3 = 0 (ct_ss_mats, SolverMPC.cpp:260-279), so with N1 = dt A_c + dt^2/2 A_c^2
//   Adt = I + N1,  Bdt = (dt I + dt^2/2 A_c + dt^3/6 A_c^2) B_c,  Qdt likewise with Q_c
// exactly; each acts as a few sparse operations, stated here once.
#pragma once
#include "cmpc_common.h"

namespace cmpc {
namespace {

// scr: [0..8] R, [9..17] I_world^-1, [18] x_drag, [19] f_est(3) term, [20..31] x_0
constexpr int kEvS0 = 32;

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

// One lane's work: R (Eigen toRotationMatrix, RobotState.cpp:36) and I_world = R I_body R'
// (SolverMPC.cpp:593; I_body = diag(ib0, ib1, ib2), the handle's model; RobotState.h:25 is the
// default) in fp64 from the fp32 quaternion, the inverse by cofactors; x_drag, the Q_c f term and
// x_0 beside them (the layout of scr above)
// rigid_frame: R, I_world^-1 and x_drag alone (scr[0..18]): what Adt and Bdt are made of. It reads
// the quaternion and x_drag words of the record and no other.
__device__ __forceinline__ void rigid_frame(const float* __restrict__ rec, double ib0, double ib1, double ib2,
                                            double* scr) {
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
  scr[18] = (double)rec[CMPC_REC_XDRAG];
}
__device__ __forceinline__ void rigid_setup(const float* __restrict__ rec, double ib0, double ib1, double ib2,
                                            double* scr) {
  rigid_frame(rec, ib0, ib1, ib2, scr);
  const uint32_t flags = __float_as_uint(rec[CMPC_REC_FLAGS]);
  scr[19] = (flags & 1u) ? (double)rec[CMPC_REC_FEST3] : 0.0;  // Q_c f (SolverMPC.cpp:808-811)
  rpy_rounded(rec, &scr[20]);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    scr[23 + i] = (double)rec[CMPC_REC_P + i];
    scr[26 + i] = (double)rec[CMPC_REC_W + i];
    scr[29 + i] = (double)rec[CMPC_REC_V + i];
  }
}

// Lane (k, a) of the first 3N: t_a = sum_f (r_f x u_kf)_a and s_a = sum_f u_kf,a over all four
// feet of step k, into ts[6k + a] and ts[6k + 3 + a]
__device__ __forceinline__ void foot_sums(int lane, int N, const float* __restrict__ rec, const float* u,
                                          double* ts) {
  if (lane < 3 * N) {
    const int k = lane / 3, a = lane - 3 * k;
    const int a1 = (a == 2) ? 0 : a + 1, a2 = (a == 0) ? 2 : a - 1;
    double tc = 0.0, sc = 0.0;
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const float* uf = &u[12 * k + 3 * f];
      // (r x u)_a = r_a1 u_a2 - r_a2 u_a1
      tc += (double)rec[CMPC_REC_R + 4 * a1 + f] * (double)uf[a2] - (double)rec[CMPC_REC_R + 4 * a2 + f] * (double)uf[a1];
      sc += (double)uf[a];
    }
    ts[6 * k + a] = tc;
    ts[6 * k + 3 + a] = sc;
  }
}

// Component j of Bdt u + Qdt f + (Adt's column of the gravity state) grav, for a step whose forces
// have the torque sum tq and the force sum sq: w = B_c u + Q_c f has w[6:9] = I_world^-1 tq and
// w[9:12] = sq / m (+ fe, the f_est(3) term, into row 9). scr as rigid_setup leaves it.
__device__ __forceinline__ double step_input(int j, const double (&tq)[3], const double (&sq)[3], double fe,
                                             double grav, const double* scr, double dt, double dth, double dt3,
                                             double im64) {
  const double* R = scr;
  const double* Ii = scr + 9;
  const double xd = scr[18];
  const double w9 = sq[0] * im64 + fe;
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
  return c;
}

// Row jj of N1 = Adt - I over the 12 dynamic states: its entries in columns 6..11 (the others are
// zero; the gravity state's are in step_input). Rows 0..2 dt R' x[6:9]; 3, 4 dt x9, x10;
// 5 dt x11 + dt^2/2 x_drag x9; 11 dt x_drag x9.
struct N1Row { double c6, c7, c8, c9, c10, c11; };
__device__ __forceinline__ N1Row n1_row(int jj, const double* scr, double dt, double dth) {
  const double* R = scr;
  N1Row r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (jj < 3) { r.c6 = dt * R[jj]; r.c7 = dt * R[3 + jj]; r.c8 = dt * R[6 + jj]; }
  if (jj == 3) r.c9 = dt;
  if (jj == 4) r.c10 = dt;
  if (jj == 5) { r.c11 = dt; r.c9 = dth * scr[18]; }
  if (jj == 11) r.c9 = dt * scr[18];
  return r;
}
// Column j of N1 as (row, value) pairs, at most three (columns 0..5 are empty; absent pairs are
// (0, 0.0)): 6 + m rows 0..2 dt R[3 m + r]; 9 rows 3, 5, 11; 10 row 4; 11 row 5. With it X N1 and
// N1'X cost three products per entry: (X N1)[i][c] = sum_t X[i][r_t(c)] v_t(c), (N1'X)[i][c] =
// sum_t v_t(i) X[r_t(i)][c].
struct N1Col { int r0, r1, r2; double v0, v1, v2; };
__device__ __forceinline__ N1Col n1_col(int j, const double* scr, double dt, double dth) {
  const double* R = scr;
  N1Col c{0, 0, 0, 0.0, 0.0, 0.0};
  if (j >= 6 && j < 9) {
    const int m = j - 6;
    c.r0 = 0; c.r1 = 1; c.r2 = 2;
    c.v0 = dt * R[3 * m]; c.v1 = dt * R[3 * m + 1]; c.v2 = dt * R[3 * m + 2];
  }
  if (j == 9) { c.r0 = 3; c.r1 = 5; c.r2 = 11; c.v0 = dt; c.v1 = dth * scr[18]; c.v2 = dt * scr[18]; }
  if (j == 10) { c.r0 = 4; c.v0 = dt; }
  if (j == 11) { c.r0 = 5; c.v0 = dt; }
  return c;
}
// Row jj of N1': its entries in columns 0..5 and 11 (rows 6..8 dt R lambda[0:3]; 9 dt (l3 +
// x_drag l11) + dt^2/2 x_drag l5; 10 dt l4; 11 dt l5)
struct N1tRow { double e0, e1, e2, e3, e4, e5, e11; };
__device__ __forceinline__ N1tRow n1t_row(int jj, const double* scr, double dt, double dth) {
  const double* R = scr;
  N1tRow r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (jj >= 6 && jj < 9) { r.e0 = dt * R[3 * (jj - 6)]; r.e1 = dt * R[3 * (jj - 6) + 1]; r.e2 = dt * R[3 * (jj - 6) + 2]; }
  if (jj == 9) { r.e3 = dt; r.e11 = dt * scr[18]; r.e5 = dth * scr[18]; }
  if (jj == 10) r.e4 = dt;
  if (jj == 11) r.e5 = dt;
  return r;
}

}  // namespace
}  // namespace cmpc
