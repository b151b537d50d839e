// cmpc_face.h — the face of the friction pyramids that given forces lie on, as cmpc_sensitivity.hip
// and cmpc_gain.hip both take it (include/cmpc_solver.h states it under cmpc_batch_sensitivity): one
// lane classifies the four foot-steps of one horizon step and lists the columns of Z_k.
#pragma once
#include "cmpc_rigid64.h"

namespace cmpc {
namespace {

// NaN-propagating minimum
__device__ __forceinline__ double nmin(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double bfly_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = nmin(v, __shfl_xor(v, m, 64));
  return v;
}

// Step k of an instance: the face of its four foot-steps at the forces u (the instance's 12 N fp32
// forces), a closed-form basis per foot-step, and the columns of Z_k (at most 12) listed as (foot,
// three coefficients): column c's foot to zf[c], its coefficients to zv[3 c .. 3 c + 2]. Every
// coefficient is 0, +-1 or +-1/mu as fmat holds it in fp32, so ZT = float stores them exactly.
// -> the number of columns; smin: the running minimum of the slacks of the inactive rows.
template <typename ZT>
__device__ __forceinline__ int face_columns(int k, int N, const float* __restrict__ rec, const float* u,
                                            const KParams& P, double act_tol, unsigned char* zf, ZT* zv,
                                            double& smin) {
  const double mu_inv = (double)P.mu_inv;  // 1/mu as fmat holds it in fp32 (SolverMPC.cpp:657)
  const double nrm = 1.0 / sqrt(mu_inv * mu_inv + 1.0);
  const unsigned char* gait = reinterpret_cast<const unsigned char*>(rec + CMPC_REC_GAIT(N));
  int col = 0;
  for (int f = 0; f < 4; f++) {
    const int t = 4 * k + f;
    // ub(fz) = gait x f_max in fp32; swing (pinned) iff |ub| < 0.01, as every solver kernel tests
    const float ubf = (float)gait[t] * P.f_max;
    if (ubf < 0.01f && ubf > -0.01f) continue;
    const double u0 = (double)u[3 * t], u1 = (double)u[3 * t + 1], u2 = (double)u[3 * t + 2];
    // the six rows of CMPC_CERT_VIOL, the friction rows normalised to unit length
    const double s0 = (u0 * mu_inv + u2) * nrm, s1 = (-u0 * mu_inv + u2) * nrm;
    const double s2 = (u1 * mu_inv + u2) * nrm, s3 = (-u1 * mu_inv + u2) * nrm;
    const double s4 = u2, s5 = (double)ubf - u2;
    const bool a0 = s0 <= act_tol, a1 = s1 <= act_tol, a2 = s2 <= act_tol, a3 = s3 <= act_tol;
    const bool a4 = s4 <= act_tol, a5 = s5 <= act_tol;
    if (!a0) smin = nmin(smin, s0);
    if (!a1) smin = nmin(smin, s1);
    if (!a2) smin = nmin(smin, s2);
    if (!a3) smin = nmin(smin, s3);
    if (!a4) smin = nmin(smin, s4);
    if (!a5) smin = nmin(smin, s5);
    // fz at 0, or both sides of an axis: the apex, nothing free
    if (a4 || (a0 && a1) || (a2 && a3)) continue;
    const bool sx = a0 || a1, sy = a2 || a3;
    const double gx = a0 ? 1.0 : -1.0, gy = a2 ? 1.0 : -1.0;  // the active side's normal (g mu_inv, ., 1)
    double z[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int d;
    if (a5) {  // the cap: fz fixed
      d = 0;
      if (!sx && !sy) { z[0] = 1.0; z[1] = 0.0; z[2] = 0.0; z[3] = 0.0; z[4] = 1.0; z[5] = 0.0; d = 2; }
      else if (sx && !sy) { z[0] = 0.0; z[1] = 1.0; z[2] = 0.0; d = 1; }
      else if (!sx && sy) { z[0] = 1.0; z[1] = 0.0; z[2] = 0.0; d = 1; }
    } else if (sx && sy) {  // an edge
      z[0] = gx; z[1] = gy; z[2] = -mu_inv; d = 1;
    } else if (sx) {
      z[0] = 0.0; z[1] = 1.0; z[2] = 0.0; z[3] = 1.0; z[4] = 0.0; z[5] = -gx * mu_inv; d = 2;
    } else if (sy) {
      z[0] = 1.0; z[1] = 0.0; z[2] = 0.0; z[3] = 0.0; z[4] = 1.0; z[5] = -gy * mu_inv; d = 2;
    } else {
      z[0] = 1.0; z[1] = 0.0; z[2] = 0.0; z[3] = 0.0; z[4] = 1.0; z[5] = 0.0; z[6] = 0.0; z[7] = 0.0; z[8] = 1.0;
      d = 3;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (c >= d) break;
      zf[col] = (unsigned char)f;
      zv[3 * col] = (ZT)z[3 * c];
      zv[3 * col + 1] = (ZT)z[3 * c + 1];
      zv[3 * col + 2] = (ZT)z[3 * c + 2];
      col++;
    }
  }
  return col;
}

}  // namespace
}  // namespace cmpc
