// cmpc_condense.hip — parity hook for the condensation rows (SolverMPC.cpp:96-146, 806-814) and
// the condensation stage of the JCQP paths (use_jcqp == 1 / 2): the full reduced-free qH [12N x
// 12N] and qg [12N] of every instance, all variables kept (no swing elimination), by the same
// structured recursions as the solver kernels (cmpc_common.h) — never forming A_qp, B_qp or the
// dense 13N x 13N weight matrix S. One 256-thread workgroup per instance, grid-strided; the
// symmetric H is written straight to the caller's buffer.
// Row-owner mode (rows): every row runs its chain on down to step 0 (below its own step k_v as
// z_i = Adt' z_{i+1}, the source term masked off) and writes its own entries on both sides of the
// diagonal, nothing mirrored: what class 1's two-stance rows compute (cmpc_class1.hip,
// the st2 path of solve_c1), here under the fp64 check of the parity hook.
// CMPC_CONDENSE_INST = 1 (this file's second unit in build.py's UNITS): the per-instance build
// for a handle with a table (cmpc_batch_set_instance_params), a kernel and a launcher of their own
// names in a unit of their own, so that this unit compiles the shared kernel exactly as before.
#ifndef CMPC_CONDENSE_INST
#define CMPC_CONDENSE_INST 0
#endif
#include "cmpc_common.h"

namespace cmpc {
namespace {

constexpr int NTG = 256;

struct SharedC {
  float BdtT[12][16];
  float traj[12 * MAXN];
  float E[MAXN][16];
  float ZE[MAXN][16];
};

// One instance: H [n x n] row-major (n = 12 N) and g [n] of rec.
__device__ void condense_one(const float* __restrict__ rec, const KParams& P, SharedC& sh,
                             float* __restrict__ H, float* __restrict__ g, bool rows) {
  const int tid = threadIdx.x;
  const int N = P.N;
  const int n = 12 * N;
  for (int t = tid; t < 12 * N; t += NTG) sh.traj[t] = rec[CMPC_REC_HDR + t];
  Model md;
  make_model(rec, P.dt, P.mdl, md);
  make_bdt<NTG>(rec, md, tid, sh.BdtT);
  CondGeo cg;
  make_cond_geo<true>(rec, md, cg);
  __syncthreads();
  float wts[13];
#pragma unroll
  for (int j = 0; j < 12; j++) wts[j] = P.wts[j];
  wts[12] = 0.f;
  if (tid < N) {  // the weighted state error we_tid = S e_tid of step tid
    float e[13];
    state_error(rec, md, tid, &sh.traj[12 * tid], e);
#pragma unroll
    for (int j = 0; j < 13; j++) sh.E[tid][j] = wts[j] * e[j];
  }
  __syncthreads();
  // the gradient's suffix moments, as in the solvers: M0 over E in place, M1 / M2 in ZE
  moment_recur(&sh.E[0][0], &sh.ZE[0][0], N, tid);
  __syncthreads();
  // variable v = 12 k + c (every foot-step kept): row v by the backward recursion of its column
  for (int v = tid; v < n; v += NTG) {
    const int kv = v / 12, cv = v - 12 * (v / 12);
    float b[13], u1[13], u2[13];
#pragma unroll
    for (int j = 0; j < 13; j++) b[j] = sh.BdtT[cv][j];
    n1_mul(md, b, u1);
    n1_mul(md, u1, u2);
    // qg = 2 B_qp' S (A_qp x0 + Q_qp f - X_d)
    g[v] = grad_from_moments(b, u1, u2, sh.E[kv], sh.ZE[kv]);
    float z[13];
#pragma unroll
    for (int j = 0; j < 13; j++) z[j] = 0.f;
    for (int i = N - 1; i >= (rows ? 0 : kv); i--) {
      const bool act = i >= kv;  // (the solvers' mask: below step kv the chain has no source term)
      const float k = (float)(i - kv);
      const float k2 = 0.5f * k * (k - 1.f);
      float gk[13];
      col_power(b, u1, u2, k, k2, gk);
#pragma unroll
      for (int j = 0; j < 13; j++) gk[j] = act ? gk[j] : 0.f;
      recur(md, wts, gk, z);
      // every foot-step is kept: all four feet, columns 12 i .. 12 i + 11 (the solvers' entry form)
      step_entries(md, cg, sh.BdtT, 15u, 12 * i, z, [&](int w, float val) {
        if (w == v) val += P.alpha2;  // qH = 2 (B'SB + alpha I), SolverMPC.cpp:806
#ifdef CMPC_DIAG_PERTURB  // diagnostic builds only: a deliberately wrong qH (shows the parity gate fails)
        val *= 1.f + CMPC_DIAG_PERTURB;
#endif
        if (rows) {
          H[(size_t)v * n + w] = val;
        } else if (w >= v) {
          H[(size_t)v * n + w] = val;
          H[(size_t)w * n + v] = val;
        }
      });
    }
  }
}

#if CMPC_CONDENSE_INST
// instance i under its table entry: the shared parameters with that entry's model, weights and 2 alpha
__global__ __launch_bounds__(NTG) void cmpc_condense_inst_kernel(const float* __restrict__ recs, int batch, KParams P,
                                                                 float* __restrict__ Hout, float* __restrict__ gout,
                                                                 int rows) {
  __shared__ SharedC sh;
  const size_t n = 12 * (size_t)P.N;
  for (int inst = blockIdx.x; inst < batch; inst += gridDim.x) {
    KParams Pi = P;
    Pi.mdl = P.inst[inst].mdl;
#pragma unroll
    for (int j = 0; j < 12; j++) Pi.wts[j] = P.inst[inst].wts[j];
    Pi.alpha2 = P.inst[inst].alpha2;
    condense_one(recs + (size_t)inst * P.rec_words, Pi, sh, Hout + inst * n * n, gout + inst * n, rows != 0);
    __syncthreads();
  }
}
#else
__global__ __launch_bounds__(NTG) void cmpc_condense_kernel(const float* __restrict__ recs, int batch, KParams P,
                                                            float* __restrict__ Hout, float* __restrict__ gout,
                                                            int rows) {
  __shared__ SharedC sh;
  const size_t n = 12 * (size_t)P.N;
  for (int inst = blockIdx.x; inst < batch; inst += gridDim.x) {
    condense_one(recs + (size_t)inst * P.rec_words, P, sh, Hout + inst * n * n, gout + inst * n, rows != 0);
    __syncthreads();
  }
}

#endif

}  // namespace

#if CMPC_CONDENSE_INST
hipError_t launch_condense_inst(const float* d_recs, int batch, const KParams& P, float* d_H, float* d_g,
                                bool rows, hipStream_t stream) {
  const int grid = batch < 2048 ? batch : 2048;
  hipLaunchKernelGGL(cmpc_condense_inst_kernel, dim3(grid), dim3(NTG), 0, stream, d_recs, batch, P, d_H, d_g,
                     rows ? 1 : 0);
  return hipGetLastError();
}
#else
hipError_t launch_condense_inst(const float* d_recs, int batch, const KParams& P, float* d_H, float* d_g,
                                bool rows, hipStream_t stream);  // this file's CMPC_CONDENSE_INST unit

hipError_t launch_condense(const float* d_recs, int batch, const KParams& P, float* d_H, float* d_g,
                           bool rows, hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  if (P.inst) return launch_condense_inst(d_recs, batch, P, d_H, d_g, rows, stream);
  const int grid = batch < 2048 ? batch : 2048;
  hipLaunchKernelGGL(cmpc_condense_kernel, dim3(grid), dim3(NTG), 0, stream, d_recs, batch, P, d_H, d_g,
                     rows ? 1 : 0);
  return hipGetLastError();
}
#endif

}  // namespace cmpc
