// cmpc_multi_model_test — a plain C++ caller of cmpc_multi_set_model (include/cmpc_multi.h; no
// Python, no torch): reads records from a file, solves them on one handle under the default model
// and under the given one (cmpc_batch_set_model), then through cmpc_multi_solve at world 1 and in
// the loopback world 2 (the peer's block goes to the root itself over RCCL) after
// cmpc_multi_set_model. Prints one JSON line: whether the model moves the single handle's forces,
// and whether every multi solve equals the single handle's solve under the model bit for bit.
//   cmpc_multi_model_test <records.f32> <batch> <horizon> <mass> <Ixx> <Iyy> <Izz>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/cmpc_multi.h"

#define CHK(x)                                                                                  \
  do {                                                                                          \
    if ((x) != 0) {                                                                             \
      std::fprintf(stderr, "%s failed: %s | %s\n", #x, cmpc_multi_last_error(), cmpc_last_error()); \
      return 1;                                                                                 \
    }                                                                                           \
  } while (0)
#define HCHK(x)                                                                                 \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) {                                                                     \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                              \
      return 1;                                                                                 \
    }                                                                                           \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 8) {
    std::fprintf(stderr, "usage: %s records.f32 batch horizon mass Ixx Iyy Izz\n", argv[0]);
    return 2;
  }
  const int B = std::atoi(argv[2]), N = std::atoi(argv[3]);
  const cmpc_model mdl{std::atof(argv[4]), {std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7])}};
  const int W = cmpc_record_words(N);
  std::vector<float> recs((size_t)B * W);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(recs.data(), sizeof(float), recs.size(), f) != recs.size()) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::fclose(f);
  cmpc_params prm{};
  prm.dt = 0.026f;
  prm.mu = 0.4f;
  prm.f_max = 120.f;
  prm.horizon = N;
  const float w[12] = {0.25f, 0.25f, 10.f, 10.f, 2.f, 50.f, 0.f, 0.f, 0.3f, 0.2f, 0.2f, 0.1f};
  std::memcpy(prm.weights, w, sizeof w);
  prm.alpha = 4e-5f;
  prm.max_iter = 100;
  HCHK(hipSetDevice(0));
  float *d_recs, *d_f;
  uint8_t* d_s;
  const size_t FC = (size_t)B * 12 * N;
  HCHK(hipMalloc(&d_recs, sizeof(float) * recs.size()));
  HCHK(hipMalloc(&d_f, sizeof(float) * FC));
  HCHK(hipMalloc(&d_s, B));
  HCHK(hipMemcpy(d_recs, recs.data(), sizeof(float) * recs.size(), hipMemcpyHostToDevice));
  hipStream_t st;
  HCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  std::vector<float> f_def(FC), f_mdl(FC), f1(FC);
  std::vector<uint8_t> s_mdl(B), s1(B);
  // reference: one handle, the default model first, then the given one
  cmpc_batch* h = nullptr;
  CHK(cmpc_batch_create(&h, &prm, B, st));
  CHK(cmpc_batch_solve(h, d_recs, B, d_f, d_s, nullptr));
  HCHK(hipStreamSynchronize(st));
  HCHK(hipMemcpy(f_def.data(), d_f, sizeof(float) * FC, hipMemcpyDeviceToHost));
  CHK(cmpc_batch_set_model(h, &mdl));
  CHK(cmpc_batch_solve(h, d_recs, B, d_f, d_s, nullptr));
  HCHK(hipStreamSynchronize(st));
  HCHK(hipMemcpy(f_mdl.data(), d_f, sizeof(float) * FC, hipMemcpyDeviceToHost));
  HCHK(hipMemcpy(s_mdl.data(), d_s, B, hipMemcpyDeviceToHost));
  cmpc_batch_destroy(h);
  const bool moves = std::memcmp(f_def.data(), f_mdl.data(), sizeof(float) * FC) != 0;
  const int dev0 = 0;
  const int devs[2] = {0, 0};
  struct Case {
    int G, flags;
    float share;
  } cases[] = {{1, 0, 0.f}, {2, CMPC_MULTI_LOOPBACK, 0.f}, {2, CMPC_MULTI_LOOPBACK, 1.f}};
  std::string js;  // printed once at the end (RCCL prints its banner to stdout)
  char buf[256];
  int n_ok = 0, n_cases = 0;
  for (const Case& c : cases) {
    cmpc_multi* m = nullptr;
    CHK(cmpc_multi_create(&m, &prm, c.G, c.G == 1 ? &dev0 : devs, B, c.share, 0, c.flags));
    CHK(cmpc_multi_set_model(m, &mdl));
    HCHK(hipMemsetAsync(d_f, 0xff, sizeof(float) * FC, st));
    HCHK(hipMemsetAsync(d_s, 0xff, B, st));
    CHK(cmpc_multi_solve(m, d_recs, B, d_f, d_s, st));
    HCHK(hipStreamSynchronize(st));
    HCHK(hipMemcpy(f1.data(), d_f, sizeof(float) * FC, hipMemcpyDeviceToHost));
    HCHK(hipMemcpy(s1.data(), d_s, B, hipMemcpyDeviceToHost));
    const bool eq = std::memcmp(f_mdl.data(), f1.data(), sizeof(float) * FC) == 0 &&
                    std::memcmp(s_mdl.data(), s1.data(), B) == 0;
    int rows[2] = {0, 0};
    cmpc_multi_rows(m, B, rows);
    std::snprintf(buf, sizeof buf, "%s{\"gpus\": %d, \"loopback\": %d, \"rows\": [%d, %d], \"bitwise\": %s}",
                  n_cases ? ", " : "", c.G, c.flags, rows[0], c.G > 1 ? rows[1] : 0, eq ? "true" : "false");
    js += buf;
    n_ok += eq;
    n_cases++;
    cmpc_multi_destroy(m);
  }
  std::fflush(stdout);
  std::printf("\n{\"batch\": %d, \"horizon\": %d, \"model_moves\": %s, \"cases\": [%s], \"all_bitwise\": %s}\n", B, N,
              moves ? "true" : "false", js.c_str(), n_ok == n_cases ? "true" : "false");
  return (n_ok == n_cases && moves) ? 0 : 3;
}
