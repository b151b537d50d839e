// cmpc_class1.hip — the hot path: fused condensation + friction-cone QP for instances with
// n <= 64 reduced force variables (every trot instance at N <= 10), one wavefront per instance.
//
// One wavefront computes one call of the reference's solve_mpc()
// (be2r_cmpc_unitree/src/controllers/convexMPC/SolverMPC.cpp:566-982):
//   stance table + swing elimination (SolverMPC.cpp:859-894), model + closed-form c2qp
//   (cmpc_common.h), condensation of the reduced qH / qg (SolverMPC.cpp:806-814), the dense
//   QP (qpOASES QProblem::init in the reference, SolverMPC.cpp:955-969) solved exactly by a
//   Goldfarb-Idnani dual active-set method, scatter to q_soln (SolverMPC.cpp:970-982).
//
// MI355X mapping:
//   * lane v owns reduced variable v: row v of H, then of the Cholesky working matrix, then
//     row v of J = L^-T, held in 65 VGPRs (slot[0..63] + the gradient border slot[64]);
//   * LDS holds one packed 64x64 upper-row matrix (8.5 KB): H during assembly, then the raw
//     Cholesky columns. Because the trailing matrix of a right-looking Cholesky stays
//     symmetric, pivot column k is "register slot[k] of every lane": ONE ds_write_b32 per step
//     publishes it, and the broadcast reads are ds_read_b128; the Cholesky's trailing sweep and
//     the active set's reflection take the broadcast from lane c's register instead, as 4x4x1
//     MFMA outer products with the A-operand broadcast;
//   * J = L^-T is solved left-looking inside the factorisation's panels: the stored columns
//     are -L's, lane v keeps x_j = J[v][j] in the registers of the finished H columns, and each
//     step adds the row sums over the finished columns (16-B broadcasts, four rows per read);
//   * the QP's triangular factor R is explicit, packed upper columns in the LDS region that held
//     L; its back substitution and re-triangularisation are readlane chains, and the J rows see
//     only straight-line Givens chains (identity rotations outside the active range);
//   * every loop over matrix columns is unrolled at compile time, so register indices are
//     constants; LDS traffic between lanes of the single wavefront needs no s_barrier.
// Everything is fp32 (the reference condenses in fp32: common_types.h:14).
#include <stdlib.h>

#include "cmpc_common.h"

// occupancy targets of the 60-wide and the 64-wide build (5 for the 60-wide measured config 3
// -18 %, r04_q)
constexpr int CMPC_W1_WAVES_60 = 4;
constexpr int CMPC_W1_WAVES_PER_EU = 4;
// chunks per group of the software-pipelined vector sweeps (piped_sweep)
constexpr int C1_PIPE_GRP = 4;

// Phase profiler (diagnostic builds only, -DCMPC_PHASE_PROF): lane 0 of every solved instance
// adds the s_memtime cycles spent in each stage to g_c1_phase (scripts/phase_prof.py).
#ifdef CMPC_PHASE_PROF
__device__ unsigned long long g_c1_phase[16];
#define C1_MARK(i)                              \
  do {                                          \
    const unsigned long long _n = clock64();    \
    ph[i] += _n - t_last;                       \
    t_last = _n;                                \
  } while (0)
// active-set loop segments [8 + i], timed from the top of the trip
#define C1_SUB(i)                               \
  do {                                          \
    const unsigned long long _n = clock64();    \
    ph[8 + (i)] += _n - t_sub;                  \
    t_sub = _n;                                 \
  } while (0)
#else
#define C1_MARK(i) \
  do {             \
  } while (0)
#define C1_SUB(i) \
  do {            \
  } while (0)
#endif

// Placement profiler (diagnostic builds only, -DCMPC_PLACE_PROF): per instance the hardware
// wave id, the XCC id and the wall-clock (100 MHz) start / end of its wavefront
// (scripts/place_prof.py).
#ifdef CMPC_PLACE_PROF
constexpr int kPlaceMax = 65536;
__device__ unsigned int g_c1_place[4 * kPlaceMax];
#endif

namespace cmpc {
namespace {

constexpr int NL = 64;  // lanes of the wavefront (per-lane LDS arrays are sized by it)

// Row width NV (60 or 64: the 60-wide build takes every instance with n <= 60, i.e. all trot
// instances at N = 10, and saves the padding columns of the 64-wide sweeps); lanes v >= NV of a
// 60-wide build own no row.
template <int NV>
struct C1Geo {
  static constexpr int NG = NV / 4;
  static constexpr int PSZ = 4 * NG * NV - 8 * NG * (NG - 1);  // packed rows r: columns [r & ~3, NV)
  // offset of packed row r (16-B aligned)
  __host__ __device__ static constexpr int prow(int r) {
    return 4 * (r >> 2) * NV - 8 * (r >> 2) * ((r >> 2) - 1) + (r & 3) * (NV - 4 * (r >> 2));
  }
  // prow(r) - (r & ~3): element (r, c) lives at prow0(r) + c
  __host__ __device__ static constexpr int prow0(int r) { return prow(r) - (r & ~3); }
  // H's exchange between the condensation and the row loads: the plain packed upper triangle,
  // element (r, c >= r) at tri(r) + c. Lane v stores its row and loads the entries c >= v at
  // tri(v) + c: with these unaligned row starts the lanes of a half-wave hit distinct banks
  // (with the 16-B aligned rows of prow, which the Cholesky's ds_read_b128 broadcasts need, only
  // 16 bank groups: 650 -> 215 extra LDS cycles per instance at NV = 60 by a bank model)
  __host__ __device__ static constexpr int tri(int r) { return r * NV - ((r * (r + 1)) >> 1); }
  static_assert(NV * NV - ((NV * (NV + 1)) >> 1) <= 4 * NG * NV - 8 * NG * (NG - 1), "exchange fits P");
};
// R (upper triangular, q x q) packed by columns: R[i][j] at rcol(j) + i, i <= j
__device__ __forceinline__ int rcol(int j) { return (j * (j + 1)) >> 1; }
// largest q whose two packed triangles fit in `words`
constexpr int rinv_cols(int words) {
  int q = 0;
  while ((q + 1) * (q + 2) <= words) q++;
  return q;
}

// prep scratch inside P (P is not yet holding H while these are live)
constexpr int OFF_E = 0;
constexpr int OFF_ZE = OFF_E + 16 * MAXN;
constexpr int OFF_REC = OFF_ZE + 16 * MAXN;  // LDS copy of the instance record (16-B aligned)

// stance foot-steps a class-1 instance can have (n = 3 x stance <= 64); the stance scan stores
// only that many (an instance with more is handed on before they are read)
constexpr int C1_MAXFS = 24;

template <int NV>
struct SharedC1 {
  static_assert(NV % 4 == 0 && NV <= NL, "row width");
  static_assert(NV * (NV + 1) / 2 <= C1Geo<NV>::PSZ, "R must fit in P");
  static_assert(OFF_REC + CMPC_REC_WORDS(MAXN) <= C1Geo<NV>::PSZ, "prep scratch must fit in P");
  static_assert(3 * C1_MAXFS >= NV, "stance list");
  // the broadcast vector (y, then the masked d / Householder vector) lives in P's last NL words
  // once J is formed: the factor rows are dead, and R (at most NV (NV + 1) / 2 words) stays below
  // it. 256 B less: the 64-wide build fits 10 KB, i.e. 16 workgroups per CU (it had 15)
  static_assert(NV * (NV + 1) / 2 <= C1Geo<NV>::PSZ - NL, "vbuf in P's tail");
  __device__ __forceinline__ float* vbuf() { return &P[C1Geo<NV>::PSZ - NL]; }
  // R^-1 (active-set phase, while the active set has at most QI positions and nothing was
  // dropped): packed by columns like R, below vbuf; R's first QI columns stay below it
  static constexpr int QI = rinv_cols(C1Geo<NV>::PSZ - NL);
  static constexpr int RB = C1Geo<NV>::PSZ - NL - QI * (QI + 1) / 2;
  static_assert(QI * (QI + 1) / 2 <= RB, "R and R^-1 side by side");
  float P[C1Geo<NV>::PSZ];
  // arrays of different stages share one region: 10 KB of LDS per instance at NV = 60, so
  // sixteen one-wave workgroups (four waves per SIMD) fit a CU's 160 KB
  union {
    float BdtT[12][16];    // prep + condensation: Bdt transposed
    struct {               // active set
      float bufA[NL], bufB[NL];  // published J rows ia (bufA) and iz (bufB + 16, running into cs)
      float cs[2 * NL];    // Givens (c, s) per column pair
    } gi;
  } u;
  float sub[C1_MAXFS];     // ub of each stance foot-step (gait * f_max): read once, into lane 3s+2
  int sfs[C1_MAXFS];       // stance foot-step ids, in order
  int blkbase[MAXN + 2];   // first reduced variable of each horizon step
  unsigned char varblk[NL], varcol[NL];
};

__device__ __forceinline__ void lsync() {
  // single-wavefront workgroup: LDS ops of one wave execute in issue order; this only stops
  // the compiler from moving LDS accesses across the point
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ float fdiv(float a, float b) { return a * fast_rcp(b); }

// The row sweeps run as broadcast MFMA outer products (mfma_chunk, cmpc_common.h). Two sweeps run
// this way here: the Cholesky's rank-2 trailing sweep and the active set's reflection update
// (profiles/r12_mfma).

// Register pin: forces every row element to be materialised at this point. Without it LLVM sinks
// the right-looking updates of slot[c] down to the step that first reads slot[c] (turning the
// factorisation left-looking in registers: O(n) multipliers and pivot values live per column,
// >1000 VGPR spills).
template <int M>
__device__ __forceinline__ void pin(float (&x)[M]) {
#pragma unroll
  for (int c = 0; c < M; c++) asm volatile("" : "+v"(x[c]));
}

// the same for the elements [C0, C1) alone
template <int C0, int C1, int M>
__device__ __forceinline__ void pin_range(float (&x)[M]) {
  static_assert(0 <= C0 && C0 <= C1 && C1 <= M, "element range");
#pragma unroll
  for (int c = C0; c < C1; c++) asm volatile("" : "+v"(x[c]));
}

// piped_sweep (cmpc_common.h) with other work under its first loads: under() runs once the first
// group's loads are issued and before any of the sweep's arithmetic, so the wave meets the LDS
// latency beneath that work. under() must not store to what ld reads.
template <int C0, int CE, int GRP, class U, class Ld, class F>
__device__ __forceinline__ void piped_sweep_under(U&& under, Ld&& ld, F&& f) {
  constexpr int NCH = (CE > C0) ? (CE - C0) / 4 : 0;
  if constexpr (NCH == 0) {
    under();
  } else {
    using T = decltype(ld(std::integral_constant<int, C0>{}));
    constexpr int NG = (NCH + GRP - 1) / GRP;
    T cur[GRP], nxt[GRP];
    static_for<0, GRP>([&](auto I) {
      constexpr int ch = decltype(I)::value;
      if constexpr (ch < NCH) cur[ch] = ld(std::integral_constant<int, C0 + 4 * ch>{});
    });
    __builtin_amdgcn_sched_barrier(0);
    under();
    static_for<0, NG>([&](auto GI) {
      constexpr int g = decltype(GI)::value;
      static_for<0, GRP>([&](auto I) {
        constexpr int ch = (g + 1) * GRP + decltype(I)::value;
        if constexpr (ch < NCH) nxt[decltype(I)::value] = ld(std::integral_constant<int, C0 + 4 * ch>{});
      });
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, GRP>([&](auto I) {
        constexpr int ch = g * GRP + decltype(I)::value;
        if constexpr (ch < NCH) f(std::integral_constant<int, C0 + 4 * ch>{}, cur[decltype(I)::value]);
      });
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, GRP>([&](auto I) { cur[decltype(I)::value] = nxt[decltype(I)::value]; });
    });
  }
}

// A value at a wave-uniform address of read-only global memory re-read where it is used, as
// karg_late does for the argument segment: a scalar load behind a pointer the optimiser cannot
// see through, so the value holds SGPRs only around its use
template <typename T>
__device__ __forceinline__ T cmem_late(const void* base, int off) {
  typedef const __attribute__((address_space(4))) char* cptr;
  cptr p = (cptr)(uintptr_t)base;
  asm volatile("" : "+s"(p));
  return *reinterpret_cast<const __attribute__((address_space(4))) T*>(p + off);
}

// step_proj (cmpc_common.h) with its derived constants passed in: dt2 = 2 dt, dtq = 2 (dt^2 / 2),
// dtc = dt^3 / 3 and imx = (1 / m) x_drag, each formed as step_proj forms it
__device__ __forceinline__ void step_proj_c(const Model& md, const CondGeo& cg, const float* z, float dt2,
                                            float dtq, float dtc, float imx, StepProj& pj) {
  const float im = md.im;
  float q[3];
#pragma unroll
  for (int i = 0; i < 3; i++)
    q[i] = fmaf(dt2, z[6 + i], dtq * fmaf(md.R[i * 3 + 2], z[2], fmaf(md.R[i * 3 + 1], z[1], md.R[i * 3] * z[0])));
#pragma unroll
  for (int j = 0; j < 3; j++)
    pj.w[j] = fmaf(cg.Ii[6 + j], q[2], fmaf(cg.Ii[3 + j], q[1], cg.Ii[j] * q[0]));
#pragma unroll
  for (int a = 0; a < 3; a++) pj.p[a] = im * fmaf(dt2, z[9 + a], dtq * z[3 + a]);
  pj.p[0] = fmaf(imx, fmaf(dtq, z[11], dtc * z[5]), pj.p[0]);
}

// Element q (LO <= q < HI, wave-uniform: an SGPR) of a register-resident row, as a tree of scalar
// branches on q with one v_mov at its leaf: no LDS traffic and almost no VALU. The opaque leaf keeps
// the optimiser from folding the branches into v_cndmask selects (HI - LO - 1 of them: measured
// slower). x[q] with a dynamic index would send the row to scratch, and so would a
// select between two elements' addresses.
template <int LO, int HI, int MA>
__device__ __forceinline__ float pick_col(const float (&x)[MA], int q) {
  static_assert(0 <= LO && LO < HI && HI <= MA, "column range");
  if constexpr (HI - LO == 1) {
    float r = x[LO];
    asm volatile("" : "+v"(r));
    return r;
  } else {
    constexpr int MID = (LO + HI) / 2;
    if (q < MID) return pick_col<LO, MID>(x, q);
    return pick_col<MID, HI>(x, q);
  }
}

// POFF, OOFF: the byte offsets of the kernel's KParams and of its three output
// pointers (forces, status, iters, one after the other) in its argument segment. The outputs are
// then read where the instance is written out (karg_late), not held in six SGPRs from kernel
// entry, and fout / st_out / it_out are not used.
// INST: the per-instance build (cmpc_batch_set_instance_params). The instance's table entry
// P.inst[inst] gives the model, f_max, 1 / mu, the weights and 2 alpha in place of P.mdl, P.f_max,
// P.mu_inv, P.wts and P.alpha2: scalar loads at a wave-uniform address (inst_late), each where the
// shared build first reads its value.
template <int NV, int POFF = -1, int OOFF = -1, bool INST = false>
__device__ __forceinline__ void solve_c1(const float* __restrict__ rec, const KParams& P,
                                         SharedC1<NV>& sh, float* __restrict__ fout,
                                         uint8_t* __restrict__ st_out, int32_t* __restrict__ it_out,
                                         int* __restrict__ ovf_list, int* __restrict__ ovf_count,
                                         int inst) {
  using G = C1Geo<NV>;
  const int v = threadIdx.x;
  const int N = P.N;
#ifdef CMPC_PHASE_PROF
  unsigned long long ph[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_sub = 0;
  unsigned long long t_last = clock64();
#endif
  // ---- stage the record in LDS: one 16-B load per lane, so the whole prep waits on a single
  // HBM round trip (record words are a multiple of 4, records 16-B aligned)
  {
    const float4* src = reinterpret_cast<const float4*>(rec);
    float4* dst = reinterpret_cast<float4*>(&sh.P[OFF_REC]);
    for (int t = v; t < (P.rec_words >> 2); t += 64) dst[t] = src[t];
  }
  lsync();
  refuse_bad_words<64>(&sh.P[OFF_REC], N, v);  // (ordered ahead of make_model by the lsync below)
  const float* srec = &sh.P[OFF_REC];
  const KInst* ie = nullptr;  // this instance's table entry (uniform)
  float f_max = P.f_max;
  if constexpr (INST) {
    ie = inst_entry(P, inst);
    f_max = inst_late<float>(ie, kInstFmaxOff);
  }
  // ---- stance table + elimination: eliminated iff |gait * f_max| < 0.01 (SolverMPC.cpp:869-894)
  const unsigned char* gait = reinterpret_cast<const unsigned char*>(srec + CMPC_REC_HDR + 12 * N);
  int nfs = 0;
  unsigned long long msk0 = 0ull, msk1 = 0ull;  // stance ballots of foot-steps 0..63, 64..127
  for (int c0 = 0; c0 < 4 * N; c0 += 64) {
    const int t = c0 + v;
    float ub = 0.f;
    bool f = false;
    if (t < 4 * N) {
      ub = (float)gait[t] * f_max;
      f = !(ub < 0.01f && ub > -0.01f);
    }
    const unsigned long long m = __ballot(f);
    if (c0 == 0) msk0 = m; else msk1 = m;
    const int pre = __popcll(m & ((1ull << v) - 1ull));
    if (f && nfs + pre < C1_MAXFS) {
      sh.sfs[nfs + pre] = t;
      sh.sub[nfs + pre] = ub;
    }
    nfs += __popcll(m);
  }
  const int n = 3 * nfs;
  if (n > NV) {  // hand the instance to the next size class
    if (v == 0 && ovf_list) ovf_list[atomicAdd(ovf_count, 1)] = inst;
    return;
  }
  lsync();
  {
    int kb = 0, kc = 0;
    if (v < n) {
      const int fs = sh.sfs[v / 3];
      kb = fs >> 2;
      kc = 3 * (fs & 3) + v % 3;
    }
    sh.varblk[v] = (unsigned char)kb;
    sh.varcol[v] = (unsigned char)kc;
    if (v <= N) {  // stance foot-steps before step v: popcounts of the ballots
      const int b0 = 4 * v, b1 = 4 * v - 64;
      const unsigned long long lo = (b0 >= 64) ? msk0 : (msk0 & ((1ull << b0) - 1ull));
      const unsigned long long hi = (b1 <= 0) ? 0ull : (msk1 & ((1ull << b1) - 1ull));
      sh.blkbase[v] = 3 * (__popcll(lo) + __popcll(hi));
    }
  }
  Model md;
  if constexpr (INST) make_model<kModelFromInst>(srec, P.dt, P.mdl, md, ie);
  else make_model(srec, P.dt, P.mdl, md);
  make_bdt<64>(srec, md, v, sh.u.BdtT);
  CondGeo cg;
  make_cond_geo<true>(srec, md, cg);
  lsync();
  float wts[13];
  cost_weights<INST>(P, ie, wts);
  if (v < N) {  // the weighted state error we_v = S e_v of step v
    float e[13];
    state_error(srec, md, v, srec + CMPC_REC_HDR + 12 * v, e);
#pragma unroll
    for (int j = 0; j < 13; j++) sh.P[OFF_E + 16 * v + j] = wts[j] * e[j];
  }
  lsync();
  // the gradient's suffix moments (cmpc_common.h): M0 over E in place, M1 / M2 in ZE
  moment_recur(&sh.P[OFF_E], &sh.P[OFF_ZE], N, v);
  lsync();
  C1_MARK(0);

  // ---- condensation: lane v builds H[v][w] for w >= v into packed P, and its gradient g_v
  const bool real = v < n;
  float gv;
  float slot[NV + 1];
  // Tables with exactly two stance feet at every step (trot, the deployed gait) and 6 N <= NV:
  // then n = 6 N, k_v = v / 6 and reduced column 6 i + 3 s + a of step i's s-th stance foot is a
  // compile-time register index, so lane v condenses its whole row (both sides of the diagonal,
  // from its own chain continued below step k_v) straight into slot[], with no H exchange through
  // the LDS and no row load. Every other table takes the exchange.
  // Decided from the stance ballots alone (wave-uniform, the record's property: the same path in
  // every batch and launch form)
  bool st2 = 6 * N <= NV;
  static_for<0, NV / 6>([&](auto IC) {
    constexpr int i = decltype(IC)::value;
    if (i < N) st2 = st2 && (__builtin_popcount(step_mask(msk0, msk1, i)) == 2);
  });
  {
    const int kv = real ? sh.varblk[v] : 0;
    const int cv = real ? sh.varcol[v] : 0;
    float b[13], u1[13], u2[13];
#pragma unroll
    for (int j = 0; j < 13; j++) b[j] = real ? sh.u.BdtT[cv][j] : 0.f;
    n1_mul(md, b, u1);
    n1_mul(md, u1, u2);
    // qg = 2 B_qp' S (A_qp x0 + Q_qp f - X_d)
    gv = grad_from_moments(b, u1, u2, &sh.P[OFF_E + 16 * kv], &sh.P[OFF_ZE + 16 * kv]);
    gv = real ? gv : 0.f;
    lsync();  // every moment read is issued before P is overwritten
    float z[13];
#pragma unroll
    for (int j = 0; j < 13; j++) z[j] = 0.f;
    if (st2) {
      // the model's uniform values in SGPRs for the unrolled steps: the row is live beside them
      Model ms;
#pragma unroll
      for (int j = 0; j < 9; j++) { ms.R[j] = rfl(md.R[j]); ms.n1r[j] = rfl(md.n1r[j]); }
      ms.dt = rfl(md.dt); ms.dth = rfl(md.dth); ms.xdrag = rfl(md.xdrag); ms.im = rfl(md.im);
#pragma unroll
      for (int j = 0; j < 3; j++) ms.ib[j] = md.ib[j];
      // step_proj's derived constants, formed once ahead of the steps (no step's condition
      // dominates the next one's, so each step formed them again) and kept in SGPRs
      const float dt2 = rfl(2.f * ms.dt), dtq = rfl(2.f * ms.dth), dtc = rfl(ms.dt * ms.dt * ms.dt / 3.f);
      const float imx = rfl(ms.im * ms.xdrag);
      static_for<0, NV / 6>([&](auto IC) {
        constexpr int i = NV / 6 - 1 - decltype(IC)::value;
        if (i < N) {
          // the same chain as below; at i < kv it goes on as z_i = Adt' z_{i+1}, and
          // 2 b_w' z_i is then H[v][w] of the lower triangle (k_w = i < k_v)
          const bool act = real && (i >= kv);
          const float k = (float)(i - kv);
          const float k2 = 0.5f * k * (k - 1.f);
          float gk[13];
          col_power(b, u1, u2, k, k2, gk);
#pragma unroll
          for (int j = 0; j < 13; j++) gk[j] = act ? gk[j] : 0.f;
          {
            // the weights re-read from the argument segment (scalar loads) in every step: held
            // from kernel entry they keep twelve SGPRs through the whole stage, which spills
            // (a per-instance build: from the instance's entry, the same way)
            kf32x4 w0, w1, w2;
            if constexpr (INST) {
              w0 = inst_late<kf32x4>(ie, kInstWtsOff);
              w1 = inst_late<kf32x4>(ie, kInstWtsOff + 16);
              w2 = inst_late<kf32x4>(ie, kInstWtsOff + 32);
            } else {
              w0 = karg_late<kf32x4>(POFF + (int)offsetof(KParams, wts));
              w1 = karg_late<kf32x4>(POFF + (int)offsetof(KParams, wts) + 16);
              w2 = karg_late<kf32x4>(POFF + (int)offsetof(KParams, wts) + 32);
            }
            const float ws[13] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, 0.f};
            recur(ms, ws, gk, z);
          }
          const float alpha2 = cost_alpha2<INST>(P, ie);
          StepProj pj;
          step_proj_c(ms, cg, z, dt2, dtq, dtc, imx, pj);
          // (the ballot opaque: the step's nibble is shifted out here, not kept from the test above)
          unsigned long long mo0 = msk0;
          asm volatile("" : "+s"(mo0));
          const unsigned mi = step_mask(mo0, 0ull, i);  // (i < 16: the first ballot alone)
          static_for<0, 2>([&](auto SC) {
            constexpr int s = decltype(SC)::value;
            // the step's s-th stance foot: lowest / next set bit of the nibble (an SGPR). Its
            // position likewise comes from the record in global memory (the values of cg.r), three
            // scalar loads at the foot's offset: no select among the twelve words
            const int f = __builtin_ctz(s == 0 ? mi : (mi & (mi - 1u)));
            const float r0 = cmem_late<float>(rec, 4 * (CMPC_REC_R + f)),
                        r1 = cmem_late<float>(rec, 4 * (CMPC_REC_R + 4 + f)),
                        r2 = cmem_late<float>(rec, 4 * (CMPC_REC_R + 8 + f));
            float val[3];
            foot_entries(pj, r0, r1, r2, val);
            static_for<0, 3>([&](auto AC) {
              constexpr int c = 6 * i + 3 * s + decltype(AC)::value;
              float x = val[decltype(AC)::value];
              if (c == v) x += alpha2;  // qH = 2 (B'SB + alpha I), SolverMPC.cpp:806
              slot[c] = real ? x : ((c == v) ? 1.f : 0.f);
            });
          });
        } else {
          static_for<6 * i, 6 * i + 6>([&](auto C) {
            constexpr int c = decltype(C)::value;
            slot[c] = (c == v) ? 1.f : 0.f;
          });
        }
        // the step's entries are formed here: nothing of the chain sinks past it
        pin_range<6 * i, 6 * i + 6>(slot);
      });
      static_for<6 * (NV / 6), NV>([&](auto C) {  // identity padding past the last whole step
        constexpr int c = decltype(C)::value;
        slot[c] = (c == v) ? 1.f : 0.f;
      });
      slot[NV] = gv;
      C1_MARK(1);
    } else {
      const int myrow = G::tri(v);
      const float alpha2 = cost_alpha2<INST>(P, ie);
      for (int i = N - 1; i >= 0; i--) {
        // z_i = S Adt^{i-kv} b_v + Adt' z_{i+1}  (the S term only for i >= kv)
        const bool act = real && (i >= kv);
        const float k = (float)(i - kv);
        const float k2 = 0.5f * k * (k - 1.f);
        float gk[13];
        col_power(b, u1, u2, k, k2, gk);
#pragma unroll
        for (int j = 0; j < 13; j++) gk[j] = act ? gk[j] : 0.f;
        recur(md, wts, gk, z);
        asm volatile("" ::: "memory");  // the step's LDS traffic stays inside the step
        const int wb = __builtin_amdgcn_readfirstlane(sh.blkbase[i]);
        step_entries(md, cg, sh.u.BdtT, step_mask(msk0, msk1, i), wb, z, [&](int w, float val) {
          if (w == v) val += alpha2;  // qH = 2 (B'SB + alpha I), SolverMPC.cpp:806
          if (act && w >= v) sh.P[myrow + w] = val;
        });
      }
      lsync();
    }
  }

  // ---- row v of H into registers (full symmetric; identity padding for v >= n) ----------
  if (!st2) {  // (the two-stance rows are in slot[] already)
    C1_MARK(1);
    const int vv = (v < NV) ? v : 0;  // lanes without a row read row 0 (and keep a zero row)
    const int myrow = G::tri(vv);
    static_for<0, NV>([&](auto C) {
      constexpr int c = decltype(C)::value;
      const int addr = (c >= vv) ? myrow + c : G::tri(c) + vv;
      const float x = sh.P[addr];
      slot[c] = (real && c < n) ? x : ((c == v) ? 1.f : 0.f);
      if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    });
    slot[NV] = gv;
    lsync();
  }

  // ---- bordered Cholesky [H | g] with J = L^-T and x = -J y solved inside it ----------------
  // Column k of the working matrix is slot[k] of every lane. Pivots come in pairs (j even, j+1):
  // a pair's rank-2 update takes the raw column j and column j+1 as it is after pivot j,
  //   slot[c] += a0 P_j[c] + a1 P_j+1[c]  (c >= j+2),  a0 = -H[v][j] / d_j,  a1 = -s1 / d_j+1,
  //   s1 = H[v][j+1] - beta H[v][j],  beta = H[j+1][j] / d_j,  d_j+1 = H[j+1][j+1] - beta H[j+1][j]
  // and look(j) forms a pair's beta / d / 1/sqrt(d) by readlane and publishes column j and the
  // corrected column j+1: one element per lane in a register (pub), and stored to P (one
  // ds_write_b32 each), where only the J sums of later panels read them. The stored columns (raw
  // even, corrected odd) are what J = L^-T needs.
  // A step is a panel of four pivots k .. k+3 (k = 0 mod 4: a sweep chunk), so NV / 4 serial steps:
  //   * pair (k, k+1) from the look before; its update of columns k+2, k+3 is two FMAs per column
  //     in the VALU, on the values lanes k+2, k+3 hold of the two published columns (what the MFMA
  //     would broadcast, and one fmaf like it), pivot k's before pivot k+1's;
  //   * look(k+2) on the now-final columns k+2, k+3, and the second pair's coefficients;
  //   * one rank-4 sweep over the chunks c >= k+4, the columns taken from the registers of the
  //     lanes that own them as MFMA outer products (mfma_chunk). The chunk at k+4 takes all four
  //     pivots first and look(k+4), the next panel's, follows it at once; the other chunks take all
  //     of pivot k, then all of k+1, k+2, k+3 (MFMAs on one accumulator a sweep apart). Every
  //     element gets its four FMAs in pivot order, as NV / 2 rank-2 steps would give them;
  //   * rows k .. k+3 of J, left-looking: their sums over the finished columns q < k read only what
  //     earlier panels stored, the triangular solve inside the panel takes its five multipliers
  //     by readlane from the published registers; their terms are added to x = -J y.
  // The second pair of a panel (the update of columns k+2, k+3, look(k+2), pivots k+2, k+3 of the
  // sweep, rows k+2, k+3 of J) runs only if k+2 < n (wave-uniform); rows and columns past n stay
  // the identity padding. Odd n: the last pair's second pivot is the identity padding row
  // (H[n][n] = 1, no coupling). The stage ends with J in slot[0..NV) and the unconstrained
  // minimiser in xunc.
  int status = CMPC_OK;
  float i0n = 1.f, betan = 0.f, i1n = 1.f, g0n = 0.f, g1n = 0.f;
  // the two published columns as look leaves them, one element per lane: the MFMA sweep's A operand
  float pub0n = 0.f, pub1n = 0.f;
  // pivot data of the step at columns (j, j+1) from the current rows, and the publish of both
  // columns (lanes >= the columns' chunk start)
  auto look = [&](auto JJ) {
    constexpr int j = decltype(JJ)::value, j1 = j + 1;
    constexpr int cj = j & ~3, cj1 = j1 & ~3;
    if constexpr (j1 < NV) {  // (also instantiated, never called, past the last step)
    float d0 = rl(slot[j], j);
    const float h10 = rl(slot[j], j1);
    if (!(d0 > 0.f)) { status = CMPC_NOT_PD; d0 = 1e-30f; }
    i0n = __builtin_amdgcn_rsqf(d0);  // d is a normal positive pivot
    betan = h10 * (i0n * i0n);
    float d1 = fmaf(-h10, betan, rl(slot[j1], j1));
    if (!(d1 > 0.f)) { status = CMPC_NOT_PD; d1 = 1e-30f; }
    i1n = __builtin_amdgcn_rsqf(d1);
    g0n = rl(slot[NV], j);
    g1n = fmaf(-betan, g0n, rl(slot[NV], j1));  // border of row j+1 after step j
    const float s1 = fmaf(-slot[j], betan, slot[j1]);
    // the factor's columns themselves, negated: P'_j = -L[:, j] = -slot[j] / sqrt(d_j) (and the
    // corrected column j+1 likewise), so the sweep and the left-looking J both read them as they are
    g0n = -g0n * i0n;
    g1n = -g1n * i1n;
    // the sweep takes the columns from these registers; the stores feed only the J sums, which
    // belong to later panels and order themselves after them (lsync at the top of a panel)
    pub0n = (v >= j) ? -slot[j] * i0n : 0.f;
    pub1n = (v >= j1) ? -s1 * i1n : 0.f;
    if (v >= cj && v < NV) sh.P[G::prow(j) + v - cj] = pub0n;
    if (v >= cj1 && v < NV) sh.P[G::prow(j1) + v - cj1] = pub1n;
    }
  };
  if (n > 0) look(std::integral_constant<int, 0>{});
  // x = -J y accumulated as J's entries are solved: y_j = -g of pivot j (the border of row j
  // after the pivots before it, scaled by -1/sqrt(d_j) in look)
  float xunc = 0.f;
  static_for<0, NV / 4>([&](auto KB) {
    constexpr int k = 4 * decltype(KB)::value;
    constexpr int k1 = k + 1, k2 = k + 2, k3 = k + 3, c4 = k + 4;
    if (k < n) {
      // (the J sums read columns stored by earlier panels: ordered after those stores here, and
      // free to move above this panel's own)
      lsync();
      const bool half2 = k2 < n;  // the second pair runs (wave-uniform)
      // the pair's uniform values in SGPRs: they stay live down to the panel's J rows
      const float i0 = rfl(i0n), i1 = rfl(i1n), g0 = rfl(g0n), g1 = rfl(g1n);
      const float p0 = pub0n, p1 = pub1n;
      const float s0 = slot[k];
      const float s1 = fmaf(-s0, betan, slot[k1]);
      // row v of L in columns k, k+1 (the sweep adds l_vk P'_k + l_vk+1 P'_k+1, P' = -L)
      const float a0 = (v > k) ? s0 * i0 : 0.f;
      const float a1 = (v > k1) ? s1 * i1 : 0.f;
      slot[NV] = fmaf(a1, g1, fmaf(a0, g0, slot[NV]));
      // the multipliers inside the panel, -L[r][c] for k <= c < r <= k+3 and c <= k+1, as lane r
      // holds them of the published columns: the in-panel update and the J rows both take them
      const float hk = rl(p0, k1);
      const float l02 = rl(p0, k2), l03 = rl(p0, k3), l12 = rl(p1, k2), l13 = rl(p1, k3);
      float i2 = 1.f, i3 = 1.f, g2 = 0.f, g3 = 0.f, hk2 = 0.f;
      float a2 = 0.f, a3 = 0.f, p2 = 0.f, p3 = 0.f;
      if (half2) {
        // columns k+2, k+3 of every lane take pivots k, k+1; then they are final
        slot[k2] = fmaf(l12, a1, fmaf(l02, a0, slot[k2]));
        slot[k3] = fmaf(l13, a1, fmaf(l03, a0, slot[k3]));
        look(std::integral_constant<int, k2>{});
        i2 = rfl(i0n); i3 = rfl(i1n); g2 = rfl(g0n); g3 = rfl(g1n);
        p2 = pub0n; p3 = pub1n;
        hk2 = rl(p2, k3);
        const float s2 = slot[k2];
        const float s3 = fmaf(-s2, betan, slot[k3]);
        a2 = (v > k2) ? s2 * i2 : 0.f;
        a3 = (v > k3) ? s3 * i3 : 0.f;
        slot[NV] = fmaf(a3, g3, fmaf(a2, g2, slot[NV]));
      }
      // slot[c] += a0 P'_k[c] + ... + a3 P'_k+3[c] with P'[c] taken from lane c's register. The
      // next panel's chunk takes every pivot first (the look-ahead follows it); the others all of
      // pivot k, then all of pivot k+1, k+2, k+3, so that two MFMAs on one accumulator sit a
      // sweep apart. Each element gets the pivots' FMAs in pivot order. The second pair's MFMAs sit
      // behind the uniform half2 (MFMAs ignore EXEC)
      if constexpr (c4 < NV) {
        mfma_chunk<c4>(p0, a0, slot[c4 + 0], slot[c4 + 1], slot[c4 + 2], slot[c4 + 3]);
        mfma_chunk<c4>(p1, a1, slot[c4 + 0], slot[c4 + 1], slot[c4 + 2], slot[c4 + 3]);
        if (half2) {
          mfma_chunk<c4>(p2, a2, slot[c4 + 0], slot[c4 + 1], slot[c4 + 2], slot[c4 + 3]);
          mfma_chunk<c4>(p3, a3, slot[c4 + 0], slot[c4 + 1], slot[c4 + 2], slot[c4 + 3]);
          if (c4 < n) look(std::integral_constant<int, c4>{});  // columns k+4, k+5 are final
        }
      }
      // (the other chunks: issued below, under the first loads of the J sums)
      const auto sweep_rest = [&]() {
        static_for<c4 / 4 + 1, NV / 4>([&](auto JC) {
          constexpr int c = 4 * decltype(JC)::value;
          mfma_chunk<c>(p0, a0, slot[c + 0], slot[c + 1], slot[c + 2], slot[c + 3]);
        });
        static_for<c4 / 4 + 1, NV / 4>([&](auto JC) {
          constexpr int c = 4 * decltype(JC)::value;
          mfma_chunk<c>(p1, a1, slot[c + 0], slot[c + 1], slot[c + 2], slot[c + 3]);
        });
        if (half2) {
          static_for<c4 / 4 + 1, NV / 4>([&](auto JC) {
            constexpr int c = 4 * decltype(JC)::value;
            mfma_chunk<c>(p2, a2, slot[c + 0], slot[c + 1], slot[c + 2], slot[c + 3]);
          });
          static_for<c4 / 4 + 1, NV / 4>([&](auto JC) {
            constexpr int c = 4 * decltype(JC)::value;
            mfma_chunk<c>(p3, a3, slot[c + 0], slot[c + 1], slot[c + 2], slot[c + 3]);
          });
        }
      };
      // J = L^-T, left-looking, four rows per 16-B read: the sums of rows k..k+3 over every
      // finished column j < k (one ds_read_b128 broadcast of P'_j[k..k+3] per column, four columns
      // per group, the next group's loads issued before this group's FMAs, two accumulators per
      // row); then the triangular solve inside the panel finishes the four rows. The sums read only
      // earlier panels' columns, so their first loads go out ahead of the sweep's other chunks
      {
        f2v t0 = {(v == k) ? 1.f : 0.f, 0.f}, t1 = {(v == k1) ? 1.f : 0.f, 0.f};
        f2v t2 = {(v == k + 2) ? 1.f : 0.f, 0.f}, t3 = {(v == k + 3) ? 1.f : 0.f, 0.f};
        piped_sweep_under<0, k, 1>(
            sweep_rest,
            [&](auto C) {
              constexpr int q = decltype(C)::value;  // columns q .. q+3 (4 | k)
              return F4x4{*reinterpret_cast<const float4*>(&sh.P[G::prow(q) + k - q]),
                          *reinterpret_cast<const float4*>(&sh.P[G::prow(q + 1) + k - q]),
                          *reinterpret_cast<const float4*>(&sh.P[G::prow(q + 2) + k - q]),
                          *reinterpret_cast<const float4*>(&sh.P[G::prow(q + 3) + k - q])};
            },
            [&](auto C, F4x4 l) {
              constexpr int q = decltype(C)::value;
              const float4 la = l.a, lb = l.b, lc = l.c, ld = l.d;
              t0.x = fmaf(slot[q], la.x, t0.x); t1.x = fmaf(slot[q], la.y, t1.x);
              t2.x = fmaf(slot[q], la.z, t2.x); t3.x = fmaf(slot[q], la.w, t3.x);
              t0.y = fmaf(slot[q + 1], lb.x, t0.y); t1.y = fmaf(slot[q + 1], lb.y, t1.y);
              t2.y = fmaf(slot[q + 1], lb.z, t2.y); t3.y = fmaf(slot[q + 1], lb.w, t3.y);
              t0.x = fmaf(slot[q + 2], lc.x, t0.x); t1.x = fmaf(slot[q + 2], lc.y, t1.x);
              t2.x = fmaf(slot[q + 2], lc.z, t2.x); t3.x = fmaf(slot[q + 2], lc.w, t3.x);
              t0.y = fmaf(slot[q + 3], ld.x, t0.y); t1.y = fmaf(slot[q + 3], ld.y, t1.y);
              t2.y = fmaf(slot[q + 3], ld.z, t2.y); t3.y = fmaf(slot[q + 3], ld.w, t3.y);
            });
        // (rows k+2, k+3 summed here: their FMAs would otherwise sink into the branch below, and
        // every loaded value stay live down to it)
        float jc2 = t2.x + t2.y, jc3 = t3.x + t3.y;
        asm volatile("" : "+v"(jc2), "+v"(jc3));
        const float xk = (t0.x + t0.y) * i0;
        slot[k] = xk;
        slot[k1] = fmaf(xk, hk, t1.x + t1.y) * i1;  // hk = -L[k+1][k]
        xunc = fmaf(slot[k1], g1, fmaf(xk, g0, xunc));
        if (half2) {  // rows k+2, k+3: the terms of columns k, k+1 on top of their sums
          const float e0 = fmaf(slot[k1], l12, fmaf(xk, l02, jc2));
          const float e1 = fmaf(slot[k1], l13, fmaf(xk, l03, jc3));
          const float xk2 = e0 * i2;
          slot[k2] = xk2;
          slot[k3] = fmaf(xk2, hk2, e1) * i3;  // hk2 = -L[k+3][k+2]
          xunc = fmaf(slot[k3], g3, fmaf(xk2, g2, xunc));
        }
      }
      pin(slot);
    }
  });
  lsync();
  C1_MARK(2);
  // (J and x = -J y are finished with the factorisation, so the profiler's phase 3 stays empty;
  // the columns past n are the identity rows' e_v already)
  C1_MARK(3);
  float xv = (v < n) ? xunc : 0.f;

  // ---- Goldfarb-Idnani dual active set on the friction pyramids -----------------------------
  // One flat loop, one active-set step per trip. The QP's triangular factor R (q x q) is kept
  // explicitly, packed by columns in P (the L rows are dead once J is formed): back substitution
  // and the re-triangularisation after a drop are readlane chains over LDS. The J rows in
  // registers see the same straight-line code on every trip — a Householder reflection (the
  // add step; beta = 0 on a drop) and an ascending Givens chain (the drop step; identity
  // rotations otherwise) — so their registers carry through the loop without copies.
  float mui = P.mu_inv;
  if constexpr (INST) mui = inst_late<float>(ie, kInstMuInvOff);
  const float fnorm = rsqrtf(mui * mui + 1.f);
  int q = 0;
  int iters = 0;
  float u_reg = 0.f;   // lane j < q: dual of active constraint j
  int act_reg = 0;     // lane j < q: id of active constraint j
  int p = -1;          // constraint being added (-1: pick the most violated one)
  Cons cp{};
  float up = 0.f;
  bool rinv_ok = true;  // R^-1 kept beside R (wave-uniform)
  lsync();
  // The selection's trip state sits in lane 3 s + 2, the lane of foot-step s's fz, which scores the
  // foot-step: its upper bound and the active flags of its six constraints (bit t). Every other lane
  // keeps all six flags set and so never offers a constraint.
  float sub_reg = 0.f;
  unsigned fm_reg = 0x3fu;
  if (v < n && v % 3 == 2) {
    sub_reg = sh.sub[v / 3];
    fm_reg = 0u;
  }
  if (status == CMPC_OK) {
    // max |x| for the selection's tolerance, taken where x changes: off the selection's chain
    float xmax = wave_max(fabsf(xv));
    for (;;) {
      pin(slot);
      const int v = tid_opq();  // re-materialised: keeps per-lane addresses out of the preheader
#ifdef CMPC_PHASE_PROF
      t_sub = clock64();
#endif
      if (p < 0) {
        // foot-step s is scored in lane 3 s + 2, which holds fz: fy and fx come down from lanes
        // 3 s + 1 and 3 s by two wave shifts (DPP: no ds_bpermute, no LDS read on this chain)
        const float fz = xv, fy = lane_prev(0.f, xv), fx = lane_prev(0.f, fy);
        float best = 0.f;
        int bid = 0x7fffffff;
        {
          float sl[6];
          sl[0] = (mui * fx + fz) * fnorm;
          sl[1] = (-mui * fx + fz) * fnorm;
          sl[2] = (mui * fy + fz) * fnorm;
          sl[3] = (-mui * fy + fz) * fnorm;
          sl[4] = fz;
          sl[5] = sub_reg - fz;
          // constraint 6 s + t = 2 (v - 2) + t in lane v = 3 s + 2
#pragma unroll
          for (int t = 0; t < 6; t++)
            if (!((fm_reg >> t) & 1u) && sl[t] < best) { best = sl[t]; bid = 2 * v - 4 + t; }
        }
        wave_argmin(best, bid);
        const float tol = 1e-5f * fmaxf(1.f, xmax);
        if (bid == 0x7fffffff || best >= -tol) break;
        p = __builtin_amdgcn_readfirstlane(bid);
        cp = decode_cons(p, mui, rl(sub_reg, 3 * (p / 6) + 2));
        up = 0.f;
      }
      C1_SUB(0);
      if (++iters > P.max_iter + 2 * n) { status = CMPC_MAX_ITER; break; }
      // d = J' n+ : rows ia, iz of J through LDS (dword stores: wide stores would tie the row
      // registers into tuples)
      if (v == cp.ia || v == cp.iz) {  // both rows in one pass (two lanes per store)
        // lane iz's row 16 words past bufB's start (into cs, written only later in a drop trip):
        // lanes ia and iz, neighbours in one half-wave, then store to different banks
        const int boff = (v == cp.iz) ? NL + 16 : 0;
#pragma unroll
        for (int c = 0; c < NV; c++) {
          sh.u.gi.bufA[boff + c] = slot[c];
          if ((c & 15) == 15) __builtin_amdgcn_sched_barrier(0);
        }
      }
      lsync();
      const float dv = (cp.ia != cp.iz) ? fmaf(cp.ca, sh.u.gi.bufA[v], cp.cb * sh.u.gi.bufB[16 + v])
                                        : cp.cb * sh.u.gi.bufB[16 + v];
      const float dm = (v >= q && v < n) ? dv : 0.f;
      sh.vbuf()[v] = dm;
      lsync();
      // z = J2 d2 (primal step direction), zn = |d2|^2 = z' n+, dn = |d|^2
      // d sits one element per lane: both norms are lane reductions, issued ahead of the z sweep
      // so that they run under its loads
      const float dn = wave_sum((v < n) ? dv * dv : 0.f);
      const float zn = wave_sum(dm * dm);
      f2v zacc = {0.f, 0.f};
      piped_sweep<0, NV, C1_PIPE_GRP>(
          [&](auto C) { return *reinterpret_cast<const float4*>(&sh.vbuf()[decltype(C)::value]); },
          [&](auto C, float4 m4) {
            constexpr int c = decltype(C)::value;
            dot4(zacc, slot[c + 0], slot[c + 1], slot[c + 2], slot[c + 3], m4);
          });
      float zv = zacc.x + zacc.y;
      // materialise the sum here: otherwise the FMAs sink below the back substitution loop and
      // the NV loaded values of vbuf stay live across it (158 VGPRs, three waves per SIMD)
      asm volatile("" : "+v"(zv));
      C1_SUB(1);
      // r = R^-1 d1 (lane i ends with r_i). While R^-1 is kept (every step so far an add, q <=
      // QI) it is a matvec over its packed columns: no dependent chain, four columns per trip.
      // Otherwise a back substitution over the packed columns of R, software-pipelined (the LDS
      // reads of step i - 1 are issued before step i's readlane / divide / FMA chain).
      float acc = dv, r_reg = 0.f;
      if (rinv_ok) {
        using S = SharedC1<NV>;
        float a0 = 0.f, a1 = 0.f;
        int j = 0;
        for (; j + 4 <= q; j += 4) {
          const float x0 = sh.P[S::RB + rcol(j) + v], x1 = sh.P[S::RB + rcol(j + 1) + v];
          const float x2 = sh.P[S::RB + rcol(j + 2) + v], x3 = sh.P[S::RB + rcol(j + 3) + v];
          a0 = fmaf((v <= j) ? x0 : 0.f, rl(dv, j), a0);
          a1 = fmaf((v <= j + 1) ? x1 : 0.f, rl(dv, j + 1), a1);
          a0 = fmaf((v <= j + 2) ? x2 : 0.f, rl(dv, j + 2), a0);
          a1 = fmaf((v <= j + 3) ? x3 : 0.f, rl(dv, j + 3), a1);
        }
        for (; j < q; j++) {
          const float x0 = sh.P[S::RB + rcol(j) + v];
          a0 = fmaf((v <= j) ? x0 : 0.f, rl(dv, j), a0);
        }
        r_reg = (v < q) ? a0 + a1 : 0.f;
      } else {
        float pd = 1.f, pv = 0.f;
        if (q > 0) {
          pd = sh.P[rcol(q - 1) + q - 1];
          pv = sh.P[rcol(q - 1) + v];
        }
        for (int i = q - 1; i >= 0; i--) {
          float pd_n = 1.f, pv_n = 0.f;
          if (i > 0) {
            pd_n = sh.P[rcol(i - 1) + i - 1];
            pv_n = sh.P[rcol(i - 1) + v];
          }
          const float ri = fdiv(rl(acc, i), pd);
          if (v < i) acc = fmaf(-pv, ri, acc);
          r_reg = (v == i) ? ri : r_reg;
          pd = pd_n;
          pv = pv_n;
        }
      }
      // partial (dual) step t1, full (primal) step t2
      float t1 = kBigF;
      int kk = 0x7fffffff;
      if (v < q && r_reg > 0.f) { t1 = fmaxf(fdiv(u_reg, r_reg), 0.f); kk = v; }
      wave_argmin(t1, kk);
      const float spv = fmaf(cp.ca, rl(xv, cp.ia), fmaf(cp.cb, rl(xv, cp.iz), -cp.bp));
      const bool zero_step = !(zn > 1e-9f * dn);
      const float t2 = zero_step ? kBigF : -fdiv(spv, zn);
      const float t = fminf(t1, t2);
      if (t >= kBigF) { status = CMPC_INFEASIBLE; break; }
      if (v < q) u_reg = fmaf(-t, r_reg, u_reg);
      up += t;
      if (!zero_step) xv = fmaf(t, zv, xv);
      xmax = wave_max(fabsf(xv));  // for the next selection: its DPP steps run under the R update's stores
      C1_SUB(2);
      const bool add = !zero_step && t2 <= t1;
      const bool add_u = __builtin_amdgcn_readfirstlane((int)add) != 0;
      float beta = 0.f, sigma = 0.f;  // w = d2 + sigma e_q
      float wreg = 0.f;  // w, one element per lane (0 on a drop): the reflection MFMAs' A operand
      if (add) {
        // ---- add p: the Householder reflection I - beta w w' on columns q..n-1 maps
        // d[q..n-1] to -sgn(d_q) |d[q..n-1]| e_q; R gains the column (d[0..q-1], -sgn ts)
        const float ts = sqrtf(zn);
        const float dq = rl(dv, q);
        const float sgn = (dq >= 0.f) ? 1.f : -1.f;
        beta = fast_rcp(ts * (ts + fabsf(dq)));  // 2 / (w'w)
        sigma = sgn * ts;
        wreg = (v == q) ? dq + sgn * ts : dm;
        const int offq = rcol(q);
        if (v < q) sh.P[offq + v] = dv;
        if (v == q) {
          sh.P[offq + q] = -sgn * ts;
          u_reg = up;
          act_reg = p;
        }
        // R^-1 gains the column (-r / rho, 1 / rho), rho = R's new diagonal: [R d1; 0 rho]^-1
        if (rinv_ok) {
          if (q < SharedC1<NV>::QI) {
            const float irho = 1.f / (-sgn * ts);
            const int offi = SharedC1<NV>::RB + rcol(q);
            if (v < q) sh.P[offi + v] = -r_reg * irho;
            if (v == q) sh.P[offi + q] = irho;
          } else {
            rinv_ok = false;
          }
        }
        if (v == cp.iz) fm_reg |= 1u << (p % 6);  // (lane 3 (p / 6) + 2 owns the foot-step's flags)
      } else {
        // ---- drop active constraint kk: shift positions kk+1..q-1 down, remove column kk of
        // R and re-triangularise rows kk..q-1 (lane c rebuilds column c of R in place: every
        // read of an old entry precedes, in this wavefront's LDS order, the write reusing it)
        const int k = __builtin_amdgcn_readfirstlane(kk);
        const int ak = rli(act_reg, k);
        if (v == 3 * (ak / 6) + 2) fm_reg &= ~(1u << (ak % 6));
        const int a_nx = lane_next_i(act_reg, act_reg);
        const float u_nx = lane_next(u_reg, u_reg);
        if (v >= k && v < q - 1) { act_reg = a_nx; u_reg = u_nx; }
        if (v < k || v > q - 2) *reinterpret_cast<float2*>(&sh.u.gi.cs[2 * v]) = make_float2(1.f, 0.f);
        const bool in_c = v >= k && v <= q - 2;
        float top = in_c ? sh.P[rcol(v + 1) + k] : 0.f;
        lsync();
        for (int r = 0; r < k; r++) {
          const float x = in_c ? sh.P[rcol(v + 1) + r] : 0.f;
          lsync();
          if (in_c) sh.P[rcol(v) + r] = x;
          lsync();
        }
        for (int j = k; j <= q - 2; j++) {
          const bool on = in_c && v >= j;
          const float bot = on ? sh.P[rcol(v + 1) + j + 1] : 0.f;
          lsync();
          const float a0 = rl(top, j), b0 = rl(bot, j);
          const float h = sqrtf(a0 * a0 + b0 * b0);
          float cc = 1.f, sn = 0.f;
          if (h > 0.f) { const float ih = fast_rcp(h); cc = a0 * ih; sn = b0 * ih; }
          if (on) {
            sh.P[rcol(v) + j] = fmaf(cc, top, sn * bot);
            top = fmaf(-sn, top, cc * bot);
          }
          if (v == 0) *reinterpret_cast<float2*>(&sh.u.gi.cs[2 * j]) = make_float2(cc, sn);
          lsync();
        }
        // R^-1 through the drop. With H = R E (column k removed) and R' = G' H restricted to its
        // first q - 1 rows (the Givens chain above), E' R^-1 is a left inverse of H, so
        //   R'^-1 = E' R^-1 G[:, 0:q-1]:
        // R^-1 without row k, the same rotations on its columns as on J's (j = k .. q-2), the
        // last column dropped. Lane i streams its row through the chain with one carried value
        // (rows i > k move up one; their entries left of column i - 1 are zero and stay so).
        if (rinv_ok) {
          using S = SharedC1<NV>;
          const int i = v;
          const bool live = i < q && i != k;
          const int i2 = (i > k) ? i - 1 : i;
          int j = (i > k) ? i - 1 : k;  // first rotation that touches row i
          float carry = (live && j >= i) ? sh.P[S::RB + rcol(j) + i] : 0.f;
          for (int jj = k; jj <= q - 2; jj++) {
            const float2 cs2 = *reinterpret_cast<const float2*>(&sh.u.gi.cs[2 * jj]);
            const float b = (live && jj >= j && jj + 1 >= i) ? sh.P[S::RB + rcol(jj + 1) + i] : 0.f;
            lsync();
            if (live && jj >= j) {
              sh.P[S::RB + rcol(jj) + i2] = fmaf(cs2.x, carry, cs2.y * b);
              carry = fmaf(-cs2.y, carry, cs2.x * b);
            }
          }
        }
      }
      lsync();
      C1_SUB(3);
      // The reflection runs on every trip (beta = 0 on a drop: a uniform branch around it costs 27
      // spilled VGPRs); the Givens chain only on a drop (add_u is wave-uniform; the branch leaves
      // the register allocation unchanged, same instruction count).
      {
        // J <- J (I - beta w w'): tw = J_v . w, J_v -= beta tw w  (no-op on a drop: beta = 0).
        // w = d2 + sigma e_q and z_v = J_v . d2 is this trip's z: tw = z_v + sigma J[v][q], one
        // column pick (scalar branches on q) and one FMA instead of a second row-long dot product
        const int qs = __builtin_amdgcn_readfirstlane(q);
        const float bt = -beta * fmaf(sigma, pick_col<0, NV>(slot, qs), zv);
        // J_v[c] += bt w[c] with w[c] from lane c's register: no store of w, no broadcast reads
        static_for<0, NV / 4>([&](auto JC) {
          constexpr int c = 4 * decltype(JC)::value;
          mfma_chunk<c>(wreg, bt, slot[c + 0], slot[c + 1], slot[c + 2], slot[c + 3]);
        });
      }
      C1_SUB(4);
      if (!add_u) {
        // J columns (j, j+1) <- Givens chain j = 0 .. NV-2 (drops only)
        static_for<0, NV - 1>([&](auto JC) {
          constexpr int j = decltype(JC)::value;
          const float2 cs2 = *reinterpret_cast<const float2*>(&sh.u.gi.cs[2 * j]);
          const float x0 = slot[j], x1 = slot[j + 1];
          slot[j] = fmaf(cs2.x, x0, cs2.y * x1);
          slot[j + 1] = fmaf(-cs2.y, x0, cs2.x * x1);
          if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        });
      }
      C1_SUB(5);
#ifdef CMPC_PHASE_PROF
      ph[14] += add ? 0ull : 1ull;
#endif
      if (add) {
        q++;
        p = -1;
      } else {
        q--;
      }
      lsync();
    }
  }

  C1_MARK(4);
  // ---- scatter (q_soln layout 12 k + 3 leg + axis, swing -> 0) staged in LDS, coalesced out
  // A solution that is no number is refused: a non-finite record word that reaches only the
  // gradient leaves every pivot positive, and a NaN never wins a comparison of the violation scan,
  // so the loop above ends "optimal" on it.
  if (status == CMPC_OK && __ballot(v < n && !result_is_number(xv)) != 0ull) status = CMPC_BAD_INPUT;
  const bool ok = (status == CMPC_OK);
  if constexpr (OOFF >= 0) {
    fout = karg_late<float*>(OOFF) + (size_t)inst * P.out_cols;
    st_out = karg_late<uint8_t*>(OOFF + 8) + inst;
    int32_t* const it_all = karg_late<int32_t*>(OOFF + 16);
    it_out = it_all ? it_all + inst : nullptr;
  }
  for (int t = v; t < 12 * N; t += 64) sh.P[t] = 0.f;
  lsync();
  if (ok && v < n) sh.P[12 * sh.varblk[v] + sh.varcol[v]] = xv;
  lsync();
  for (int t = 4 * v; t < P.out_cols; t += 256)  // (the leading steps kept, 12 N by default)
    *reinterpret_cast<float4*>(&fout[t]) = *reinterpret_cast<const float4*>(&sh.P[t]);
  if (v == 0) {
    st_out[0] = (uint8_t)status;
    if (it_out) it_out[0] = iters;
  }
#ifdef CMPC_PHASE_PROF
  C1_MARK(5);
  if (v == 0) {
    ph[6] = 1;
    ph[7] = (unsigned long long)iters;
#pragma unroll
    for (int i = 0; i < 16; i++) atomicAdd(&g_c1_phase[i], ph[i]);
  }
#endif
}

}  // namespace

// the per-instance build of the kernel below (its body with solve_c1's INST set; a kernel of its
// own name, so the shared build keeps its name and its registers)
template <int NV>
__global__ __launch_bounds__(64, NV == 60 ? CMPC_W1_WAVES_60 : CMPC_W1_WAVES_PER_EU) void cmpc_solve_c1_inst_kernel(
    const float* __restrict__ recs, int batch, KParams P, float* __restrict__ forces,
    uint8_t* __restrict__ status, int32_t* __restrict__ iters, const int* __restrict__ in_list,
    const int* __restrict__ in_count, int* __restrict__ ovf_list, int* __restrict__ ovf_count) {
  __shared__ SharedC1<NV> sh;
  int t = blockIdx.x;
  if (in_list) {
    if (t >= *in_count) return;
    t = in_list[t];
  } else if (t >= batch) {
    return;
  }
  using K = decltype(&cmpc_solve_c1_inst_kernel<NV>);
  using KP = KArg<2, K>;
  static_assert(std::is_same<typename KP::type, KParams>::value, "argument 2 is the KParams");
  static_assert(std::is_same<typename KArg<3, K>::type, float*>::value &&
                    std::is_same<typename KArg<4, K>::type, uint8_t*>::value &&
                    std::is_same<typename KArg<5, K>::type, int32_t*>::value &&
                    KArg<4, K>::offset() == KArg<3, K>::offset() + 8 &&
                    KArg<5, K>::offset() == KArg<3, K>::offset() + 16,
                "arguments 3..5 are forces, status, iters");
  solve_c1<NV, KP::offset(), KArg<3, K>::offset(), true>(recs + (size_t)t * P.rec_words, P, sh, nullptr, nullptr,
                                                         nullptr, ovf_list, ovf_count, t);
}

template <int NV>
__global__ __launch_bounds__(64, NV == 60 ? CMPC_W1_WAVES_60 : CMPC_W1_WAVES_PER_EU) void cmpc_solve_c1_kernel(
    const float* __restrict__ recs, int batch, KParams P, float* __restrict__ forces,
    uint8_t* __restrict__ status, int32_t* __restrict__ iters, const int* __restrict__ in_list,
    const int* __restrict__ in_count, int* __restrict__ ovf_list, int* __restrict__ ovf_count) {
  // one instance per workgroup, no grid-stride loop: a loop around the solve would let LICM
  // hoist hundreds of lane-invariant addresses / masks out of it and spill them
  __shared__ SharedC1<NV> sh;
  int t = blockIdx.x;
  if (in_list) {  // list mode: workgroup i takes list entry i (surplus workgroups exit)
    if (t >= *in_count) return;
    t = in_list[t];
  } else if (t >= batch) {
    return;
  }
#ifdef CMPC_PLACE_PROF
  const unsigned long long t_start = wall_clock64();
  const unsigned hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
  const unsigned xcc_id = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
#endif
  using KP = KArg<2, decltype(&cmpc_solve_c1_kernel<NV>)>;  // the KParams argument, located by this signature
  static_assert(std::is_same<typename KP::type, KParams>::value, "argument 2 is the KParams");
  using K = decltype(&cmpc_solve_c1_kernel<NV>);
  static_assert(std::is_same<typename KArg<3, K>::type, float*>::value &&
                    std::is_same<typename KArg<4, K>::type, uint8_t*>::value &&
                    std::is_same<typename KArg<5, K>::type, int32_t*>::value &&
                    KArg<4, K>::offset() == KArg<3, K>::offset() + 8 &&
                    KArg<5, K>::offset() == KArg<3, K>::offset() + 16,
                "arguments 3..5 are forces, status, iters");
  solve_c1<NV, KP::offset(), KArg<3, K>::offset()>(recs + (size_t)t * P.rec_words, P, sh, nullptr, nullptr,
                                                   nullptr, ovf_list, ovf_count, t);
#ifdef CMPC_PLACE_PROF
  const unsigned long long t_end = wall_clock64();
  if (threadIdx.x == 0 && t < kPlaceMax) {
    g_c1_place[4 * t + 0] = hw_id;
    g_c1_place[4 * t + 1] = xcc_id;
    g_c1_place[4 * t + 2] = (unsigned)t_start;
    g_c1_place[4 * t + 3] = (unsigned)t_end;
  }
#endif
}

hipError_t launch_class1(int nv, const float* d_recs, int batch, const KParams& P, float* d_forces,
                         uint8_t* d_status, int32_t* d_iters, const int* in_list, const int* in_count,
                         int* ovf_list, int* ovf_count, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  // CMPC_C1_DYN_LDS=<bytes> (diagnostic build only): extra dynamic LDS per workgroup, i.e. fewer class-1
  // workgroups per CU (placement / occupancy experiments)
  static const unsigned dyn = (unsigned)diag_knob("CMPC_C1_DYN_LDS", 0);
  if (P.inst) {  // the per-instance builds
    if (nv == 60)
      hipLaunchKernelGGL(cmpc_solve_c1_inst_kernel<60>, dim3(grid), dim3(64), dyn, stream, d_recs, batch, P,
                         d_forces, d_status, d_iters, in_list, in_count, ovf_list, ovf_count);
    else
      hipLaunchKernelGGL(cmpc_solve_c1_inst_kernel<64>, dim3(grid), dim3(64), dyn, stream, d_recs, batch, P,
                         d_forces, d_status, d_iters, in_list, in_count, ovf_list, ovf_count);
    return hipGetLastError();
  }
  if (nv == 60)
    hipLaunchKernelGGL(cmpc_solve_c1_kernel<60>, dim3(grid), dim3(64), dyn, stream, d_recs, batch, P,
                       d_forces, d_status, d_iters, in_list, in_count, ovf_list, ovf_count);
  else
    hipLaunchKernelGGL(cmpc_solve_c1_kernel<64>, dim3(grid), dim3(64), dyn, stream, d_recs, batch, P,
                       d_forces, d_status, d_iters, in_list, in_count, ovf_list, ovf_count);
  return hipGetLastError();
}

}  // namespace cmpc

#ifdef CMPC_PHASE_PROF
// cycles per stage summed over solved class-1 instances: prep, condensation, Cholesky, J,
// active set (incl. x = -J y), scatter; [6] instances, [7] active-set iterations. Resets.
extern "C" int cmpc_debug_phase_read(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_c1_phase), sizeof(unsigned long long) * 16) != hipSuccess)
    return -1;
  unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_c1_phase), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

#ifdef CMPC_PLACE_PROF
// per instance [hw_id, xcc_id, start, end] of the last class-1 launches (instances < 65536)
extern "C" int cmpc_debug_place_read(unsigned int* out, int n) {
  if (n > kPlaceMax) n = kPlaceMax;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_c1_place), sizeof(unsigned int) * 4 * n) == hipSuccess ? 0 : -1;
}
#endif
