// cmpc_mfma_probe — the register layout and rounding of v_mfma_f32_4x4x1_16b_f32 with the
// A-operand broadcast (cbsz 4, abid b), as the class-1 row sweeps use it (cmpc_class1.hip,
// mfma_chunk): one wavefront, for every abid 0..15
//   D(lane v, register i) = A(lane 4 abid + i) * B(lane v) + C(lane v, register i)
// is compared in every lane and register with the host's fmaf. Two input sets: normal values
// with zeros and negatives mixed in, and one whose inputs, addends or products are denormal.
// usage: cmpc_mfma_probe  -> one JSON line
//   layout_ok: every element of the normal set within 1e-6 relative of the fmaf
//   bitwise_fma: the normal set bit for bit;  bitwise_fma_denormals: the denormal set bit for bit
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef float f4v __attribute__((ext_vector_type(4)));

template <int AB>
__device__ __forceinline__ void one(float a, float b, const f4v c, float* __restrict__ d, int v) {
  const f4v r = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, AB, 0);
  for (int i = 0; i < 4; i++) d[(AB * 64 + v) * 4 + i] = r[i];
}

// one wavefront, no divergence: the MFMAs run with every lane enabled
__global__ __launch_bounds__(64) void probe_kernel(const float* __restrict__ A,
                                                   const float* __restrict__ B,
                                                   const float* __restrict__ C,
                                                   float* __restrict__ D) {
  const int v = threadIdx.x;
  const float a = A[v], b = B[v];
  f4v c;
  for (int i = 0; i < 4; i++) c[i] = C[4 * v + i];
  one<0>(a, b, c, D, v);   one<1>(a, b, c, D, v);   one<2>(a, b, c, D, v);   one<3>(a, b, c, D, v);
  one<4>(a, b, c, D, v);   one<5>(a, b, c, D, v);   one<6>(a, b, c, D, v);   one<7>(a, b, c, D, v);
  one<8>(a, b, c, D, v);   one<9>(a, b, c, D, v);   one<10>(a, b, c, D, v);  one<11>(a, b, c, D, v);
  one<12>(a, b, c, D, v);  one<13>(a, b, c, D, v);  one<14>(a, b, c, D, v);  one<15>(a, b, c, D, v);
}

namespace {

uint32_t rng_state = 0x9e3779b9u;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}
float unif(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) * (1.f / 16777216.f); }

uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

#define HIP_OK(x)                                                              \
  do {                                                                         \
    const hipError_t e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                                    \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));             \
      return false;                                                            \
    }                                                                          \
  } while (0)

// runs the 16 broadcasts on one input set; counts elements off by more than `rel` and elements
// whose bits differ from fmaf's
bool run_set(const std::vector<float>& A, const std::vector<float>& B, const std::vector<float>& C,
             float* dA, float* dB, float* dC, float* dD, int& n_far, int& n_bits) {
  std::vector<float> D(16 * 64 * 4);
  HIP_OK(hipMemcpy(dA, A.data(), 64 * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dB, B.data(), 64 * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dC, C.data(), 256 * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dD, 0xff, D.size() * 4));
  hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
  n_far = n_bits = 0;
  for (int ab = 0; ab < 16; ab++)
    for (int v = 0; v < 64; v++)
      for (int i = 0; i < 4; i++) {
        const float want = std::fmaf(A[4 * ab + i], B[v], C[4 * v + i]);
        const float got = D[(ab * 64 + v) * 4 + i];
        const float scale = std::fmax(std::fabs(A[4 * ab + i] * B[v]), std::fabs(C[4 * v + i]));
        if (!(std::fabs(got - want) <= 1e-6f * scale)) n_far++;
        if (bits(got) != bits(want)) n_bits++;
      }
  return true;
}

}  // namespace

int main() {
  float *dA, *dB, *dC, *dD;
  if (hipMalloc(&dA, 64 * 4) != hipSuccess || hipMalloc(&dB, 64 * 4) != hipSuccess ||
      hipMalloc(&dC, 256 * 4) != hipSuccess || hipMalloc(&dD, 16 * 64 * 4 * 4) != hipSuccess) {
    std::fprintf(stderr, "hipMalloc failed\n");
    return 1;
  }
  std::vector<float> A(64), B(64), C(256);
  // normal set: magnitudes over a few decades, both signs, a zero every seventh element
  for (int v = 0; v < 64; v++) {
    A[v] = (v % 7 == 3) ? 0.f : unif(-1.f, 1.f) * std::exp2f(unif(-6.f, 6.f));
    B[v] = (v % 7 == 5) ? 0.f : unif(-1.f, 1.f) * std::exp2f(unif(-6.f, 6.f));
  }
  for (int t = 0; t < 256; t++) C[t] = (t % 7 == 1) ? 0.f : unif(-1.f, 1.f) * std::exp2f(unif(-6.f, 6.f));
  int far_n = 0, bits_n = 0;
  if (!run_set(A, B, C, dA, dB, dC, dD, far_n, bits_n)) return 1;
  // denormal set: A denormal in every fourth lane and tiny-normal elsewhere, B around 1 or tiny
  // (products denormal or underflowing), C zero, denormal or tiny-normal
  for (int v = 0; v < 64; v++) {
    A[v] = (v % 4 == 0) ? unif(-1.f, 1.f) * 1e-39f : unif(-1.f, 1.f) * 1e-30f;
    B[v] = (v % 3 == 0) ? unif(-2.f, 2.f) : unif(-1.f, 1.f) * 1e-9f;
  }
  for (int t = 0; t < 256; t++)
    C[t] = (t % 3 == 0) ? 0.f : (t % 3 == 1) ? unif(-1.f, 1.f) * 1e-40f : unif(-1.f, 1.f) * 1e-37f;
  int dfar_n = 0, dbits_n = 0;
  if (!run_set(A, B, C, dA, dB, dC, dD, dfar_n, dbits_n)) return 1;
  std::printf("{\"layout_ok\": %s, \"bitwise_fma\": %s, \"bitwise_fma_denormals\": %s, "
              "\"elements\": %d, \"far\": %d, \"bit_diffs\": %d, \"denormal_bit_diffs\": %d}\n",
              far_n == 0 ? "true" : "false", bits_n == 0 ? "true" : "false",
              dbits_n == 0 ? "true" : "false", 16 * 64 * 4, far_n, bits_n, dbits_n);
  (void)hipFree(dA);
  (void)hipFree(dB);
  (void)hipFree(dC);
  (void)hipFree(dD);
  return 0;
}
