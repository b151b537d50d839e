// cmpc_inst_table.hip — the per-instance table (cmpc_batch_set_instance_params,
// cmpc_batch_set_instance_costs): checking the caller's rows and converting them to the kernel-side
// entries.
#include <math.h>

#include "cmpc_kernels.h"

namespace cmpc {

// ---------------------------------------------------------------------------------------------
// The per-instance table (cmpc_batch_set_instance_params): rows of CMPC_INST_WORDS doubles ->
// entries of KInst. Both kernels one thread per row. The derived values are the expressions of
// make_kmodel and make_kparams (cmpc_abi.cpp) in the same order and types; this unit is compiled
// with the flags of every other one (IEEE division in both precisions, fp32 denormals kept), so a
// row equal to a handle's model and parameters gives that handle's bits.
// ---------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ KInst inst_from_row(const double* __restrict__ row) {
  KInst e;
  const double mass = row[CMPC_INST_MASS];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double ib = row[CMPC_INST_INERTIA + i];
    e.mdl.ib[i] = (float)ib;
    e.mdl.iinv64[i] = 1.0 / ib;
  }
  e.mdl.im = 1.f / (float)mass;
  e.mdl.im64 = 1.0 / mass;
  e.mu_inv = 1.f / (float)row[CMPC_INST_MU];
  e.f_max = (float)row[CMPC_INST_FMAX];
  e.pad[0] = 0.f;
  e.pad[1] = 0.f;
  return e;
}
// the first 64-byte line of an entry (the second belongs to the cost table or the shared fill)
__device__ __forceinline__ void store_model_line(KInst* __restrict__ dst, const KInst& e) {
  dst->mdl = e.mdl;
  dst->mu_inv = e.mu_inv;
  dst->f_max = e.f_max;
  dst->pad[0] = 0.f;
  dst->pad[1] = 0.f;
}

__device__ __forceinline__ bool fin64(double v) { return v == v && fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ bool fin32(float v) { return v == v && fabsf(v) <= 3.402823466e38f; }

// a row cmpc_batch_set_model (model_ok) or the table's own rules for mu and f_max refuse
__device__ __forceinline__ bool inst_row_bad(const double* __restrict__ row) {
  bool ok = true;
#pragma unroll
  for (int w = 0; w < CMPC_INST_WORDS; w++) ok = ok && fin64(row[w]);
  // mass and inertia: finite and positive, in double and after the fp32 kernels' cast ...
#pragma unroll
  for (int w = CMPC_INST_MASS; w < CMPC_INST_INERTIA + 3; w++)
    ok = ok && row[w] > 0.0 && fin32((float)row[w]) && (float)row[w] > 0.f;
  // ... and every value derived from them (a denormal mass or inertia has an infinite reciprocal)
  const KInst e = inst_from_row(row);
  ok = ok && fin32(e.mdl.im) && e.mdl.im > 0.f && fin64(e.mdl.im64) && e.mdl.im64 > 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) ok = ok && fin64(e.mdl.iinv64[i]) && e.mdl.iinv64[i] > 0.0;
  // mu: positive, with a finite positive fp32 reciprocal (fmat's 1 / mu); f_max: finite in fp32
  // (zero and below the elimination threshold are legal: every foot-step of the instance swings)
  ok = ok && row[CMPC_INST_MU] > 0.0 && fin32(e.mu_inv) && e.mu_inv > 0.f && fin32(e.f_max);
  return !ok;
}

__global__ __launch_bounds__(256) void cmpc_inst_check_kernel(const double* __restrict__ rows, int count,
                                                              int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool b = i < count && inst_row_bad(rows + (size_t)i * CMPC_INST_WORDS);
  const unsigned long long m = __ballot(b);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(bad, __popcll(m));
}

__global__ __launch_bounds__(256) void cmpc_inst_convert_kernel(const double* __restrict__ rows, int count,
                                                                KInst* __restrict__ entries,
                                                                double* __restrict__ snapshot) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const double* row = rows + (size_t)i * CMPC_INST_WORDS;
  store_model_line(entries + i, inst_from_row(row));
#pragma unroll
  for (int w = 0; w < CMPC_INST_WORDS; w++) snapshot[(size_t)i * CMPC_INST_WORDS + w] = row[w];
}

// ---- the cost table (cmpc_batch_set_instance_costs): rows of CMPC_COST_WORDS floats -> the second
// line of the entries. alpha2 is make_kparams' expression, 2.f * alpha; words 13..15 are not read.
__device__ __forceinline__ bool cost_row_bad(const float* __restrict__ row) {
  bool ok = true;
#pragma unroll
  for (int w = 0; w < 12; w++) ok = ok && fin32(row[CMPC_COST_WEIGHTS + w]) && !(row[CMPC_COST_WEIGHTS + w] < 0.f);
  const float alpha = row[CMPC_COST_ALPHA];
  ok = ok && fin32(alpha) && alpha > 0.f && fin32(2.f * alpha);
  return !ok;
}

__global__ __launch_bounds__(256) void cmpc_cost_check_kernel(const float* __restrict__ rows, int count,
                                                              int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool b = i < count && cost_row_bad(rows + (size_t)i * CMPC_COST_WORDS);
  const unsigned long long m = __ballot(b);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(bad, __popcll(m));
}

__device__ __forceinline__ void store_cost_line(KInst* __restrict__ dst, const float* w, float alpha2, float alpha) {
#pragma unroll
  for (int j = 0; j < 12; j++) dst->wts[j] = w[j];
  dst->alpha2 = alpha2;
  dst->pad2 = 0.f;
  dst->alpha64 = (double)alpha;
}

__global__ __launch_bounds__(256) void cmpc_cost_convert_kernel(const float* __restrict__ rows, int count,
                                                                KInst* __restrict__ entries) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const float* row = rows + (size_t)i * CMPC_COST_WORDS;
  float w[12];
#pragma unroll
  for (int j = 0; j < 12; j++) w[j] = row[CMPC_COST_WEIGHTS + j];
  const float alpha = row[CMPC_COST_ALPHA];
  store_cost_line(entries + i, w, 2.f * alpha, alpha);
}

// ---- the half of the entries that has no table of its own: the handle's shared values, as the
// host derived them (P), so such an entry gives the bits of the shared builds
struct InstFill {
  KModel mdl;
  float mu_inv, f_max;
  float wts[12];
  float alpha2, alpha;
  double row[CMPC_INST_WORDS];  // what a row of cmpc_batch_set_instance_params would hold
};

__global__ __launch_bounds__(256) void cmpc_inst_fill_kernel(KInst* __restrict__ entries,
                                                             double* __restrict__ snapshot, int count,
                                                             int model, InstFill f) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  if (model) {
    KInst e;
    e.mdl = f.mdl;
    e.mu_inv = f.mu_inv;
    e.f_max = f.f_max;
    store_model_line(entries + i, e);
#pragma unroll
    for (int w = 0; w < CMPC_INST_WORDS; w++) snapshot[(size_t)i * CMPC_INST_WORDS + w] = f.row[w];
  } else {
    store_cost_line(entries + i, f.wts, f.alpha2, f.alpha);
  }
}

}  // namespace

hipError_t launch_inst_check(const double* d_rows, int count, int* d_bad, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(cmpc_inst_check_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, d_rows, count, d_bad);
  return hipGetLastError();
}

hipError_t launch_inst_convert(const double* d_rows, int count, KInst* d_entries, double* d_snapshot,
                               hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(cmpc_inst_convert_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, d_rows, count,
                     d_entries, d_snapshot);
  return hipGetLastError();
}

hipError_t launch_cost_check(const float* d_rows, int count, int* d_bad, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(cmpc_cost_check_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, d_rows, count, d_bad);
  return hipGetLastError();
}

hipError_t launch_cost_convert(const float* d_rows, int count, KInst* d_entries, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(cmpc_cost_convert_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, d_rows, count,
                     d_entries);
  return hipGetLastError();
}

hipError_t launch_inst_fill(KInst* d_entries, double* d_snapshot, int count, bool model, const KParams& P,
                            const cmpc_model& mdl64, double mu, double f_max, float alpha, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  InstFill f;
  f.mdl = P.mdl;
  f.mu_inv = P.mu_inv;
  f.f_max = P.f_max;
  for (int j = 0; j < 12; j++) f.wts[j] = P.wts[j];
  f.alpha2 = P.alpha2;
  f.alpha = alpha;
  f.row[CMPC_INST_MASS] = mdl64.mass;
  for (int j = 0; j < 3; j++) f.row[CMPC_INST_INERTIA + j] = mdl64.inertia[j];
  f.row[CMPC_INST_MU] = mu;
  f.row[CMPC_INST_FMAX] = f_max;
  hipLaunchKernelGGL(cmpc_inst_fill_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, d_entries, d_snapshot,
                     count, model ? 1 : 0, f);
  return hipGetLastError();
}

}  // namespace cmpc
