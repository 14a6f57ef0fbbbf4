// kura_kernels.hip -- fused CDNA4 (gfx950) kernels for the batched Kuramoto
// environment: one launch = one SpatialKuramoto.step() (env.py:415-454) or
// one reset() transient (env.py:594-614) for every environment of a handle.
//
// Work decomposition:
//   * one workgroup = 16 environments (E_WG), 512 threads = 8 wavefronts;
//   * the O(N^2) coupling of one RHS sweep is the GEMM
//         [sin theta ; cos theta] (32 x N)  x  alpha^T (N x N)
//     on v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fmaf chain), with the
//     32 x N operand resident in LDS (132 KiB at N=1024) in MFMA fragment order
//     and alpha streamed from L2/MALL in a host-swizzled fragment layout
//     through raw buffer loads;
//   * every element-wise stage (Dopri5 stage inputs, coupling epilogue, error
//     norm, dense output + LFP, FSAL) runs in the MFMA accumulator layout:
//     wave w owns column tiles w*TPW .. w*TPW+TPW-1 for all 16 envs, and its
//     solver records ([slot][N][16 envs] in HBM) are only ever touched by the
//     lane that owns them; sums over oscillators use the RM order and sums
//     over the window the R64 order (kura_detmath.h).
// The arithmetic is a bit-exact twin of oracle/kura_oracle.c; this file must
// be compiled with -ffp-contract=off (see __graft_entry__.build).

// Build switches of settled experiments: their code is gone (DESIGN.md section
// 5, "Retired build switches": what each did, its result, where the A/B is
// kept).  A command line that still passes one must not build the product and
// label it a variant.
#if defined(KURA_EXP_ALPHA) || defined(KURA_EXP_ORDER) || defined(KURA_EXP_NO_B1) || defined(KURA_EXP_NO_B2) || \
    defined(KURA_SPLIT_SCALAR) || defined(KURA_SI_PACKED) || defined(KURA_GROUPSUM_ATOMIC) ||                   \
    defined(KURA_FUSED_ERR) || defined(KURA_SAVE_PACKED) || defined(KURA_SOLVE_INLINE) ||                       \
    defined(KURA_RESET_DEDUP) || defined(KURA_REC_LD_AUX) || defined(KURA_REC_ST_AUX) || defined(KURA_BITSEL)
#error "retired build switch (KURA_EXP_ALPHA, KURA_EXP_ORDER, KURA_EXP_NO_B1, KURA_EXP_NO_B2, KURA_SPLIT_SCALAR, KURA_SI_PACKED, KURA_GROUPSUM_ATOMIC, KURA_FUSED_ERR, KURA_SAVE_PACKED, KURA_SOLVE_INLINE, KURA_RESET_DEDUP, KURA_REC_LD_AUX, KURA_REC_ST_AUX, KURA_BITSEL): see DESIGN.md, 'Retired build switches'"
#endif

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kura.h"
#include "kura_detmath.h"

#pragma clang fp contract(off)

#define E_WG 16
#define NWAVES 8
#define NTHREADS (NWAVES * 64)
#define ENVS_PER_WAVE (E_WG / NWAVES)

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));

// ---- Dopri5 tableau cast to fp32 (identical constants to the oracle) -------
// kA[s][j]: stage s input = y0 + chain_j(kA[s][j] * k_j); kE: error weights;
// kM: dense-output mid-point weights (diffrax _Dopri5Interpolation.c_mid).
#define KF(x) ((float)(x))
__device__ constexpr float kA[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {KF(1.0 / 5.0), 0, 0, 0, 0, 0},
    {KF(3.0 / 40.0), KF(9.0 / 40.0), 0, 0, 0, 0},
    {KF(44.0 / 45.0), KF(-56.0 / 15.0), KF(32.0 / 9.0), 0, 0, 0},
    {KF(19372.0 / 6561.0), KF(-25360.0 / 2187.0), KF(64448.0 / 6561.0), KF(-212.0 / 729.0), 0, 0},
    {KF(9017.0 / 3168.0), KF(-355.0 / 33.0), KF(46732.0 / 5247.0), KF(49.0 / 176.0), KF(-5103.0 / 18656.0), 0},
    {KF(35.0 / 384.0), 0, KF(500.0 / 1113.0), KF(125.0 / 192.0), KF(-2187.0 / 6784.0), KF(11.0 / 84.0)}};
__device__ constexpr float kE[7] = {KF(35.0 / 384.0 - 1951.0 / 21600.0), 0,
                                    KF(500.0 / 1113.0 - 22642.0 / 50085.0), KF(125.0 / 192.0 - 451.0 / 720.0),
                                    KF(-2187.0 / 6784.0 + 12231.0 / 42400.0), KF(11.0 / 84.0 - 649.0 / 6300.0),
                                    KF(-1.0 / 60.0)};
__device__ constexpr float kM[7] = {KF(6025192743.0 / 30085553152.0 / 2.0), 0,
                                    KF(51252292925.0 / 65400821598.0 / 2.0),
                                    KF(-2691868925.0 / 45128329728.0 / 2.0),
                                    KF(187940372067.0 / 1594534317056.0 / 2.0),
                                    KF(-1776094331.0 / 19743644256.0 / 2.0), KF(11237099.0 / 235043384.0 / 2.0)};
#undef KF

// Everything a launch needs, passed by value (kernarg).
struct DevParams {
    int N, B, W, n_elec, n_rec, rec_kernel, reward_kind, episode_steps, max_steps, n_bins, padlen;
    int bins[KURA_MAX_BINS];
    double dt, width, pause, transient_len, act_lo, act_hi, dbs_lo, dbs_hi;
    double bw_b[5], bw_a[5], bw_zi[4];
    float rtol, atol, kn, dt0;
    const float* alpha_sw;  // B-fragment swizzled coupling
    const float* alpha_dd;  // BF16X3, N <= 1024: the deduplicated image too (the reset's GEMM, coupling_gemm_bf16x3_dd)
    unsigned alpha_dd_bytes;  // its size (the GEMM's descriptor range)
    int alpha_reuse;        // BF16X3, N = 1024: alpha has the shift structure (coupling_gemm_bf16x3_shift)
    const float* omega;     // [B][N]
    const float* kn_env;    // [B] float32(K_b / N), per-env coupling gain
    const double* g_stim;   // [B][n_elec][N]
    const double* g_rec;    // [B][N] recorder conductance sum G = g_0 + g_1 + ... (host-summed)
    const double* ctab;     // [n_bins][W]
    const double* stab;
    float* y;               // [B][N] phase state (last saved row)
    double* t;              // [B] current_time
    int* step;              // [B]
    double* ring;           // [B][W] observation window ring
    int* wpos;              // [B] next write slot == oldest sample
    float* R;               // [B/16][NSLOT][N][16] solver workspace: per slot, 16 envs per oscillator
    float* pulse;           // [B][N]
    const double* r2c;      // [W] R2 filter functional c: filtfilt(x)[-1] - mean = c . x (kura_r2.h)
    double* spec;           // [B][2 n_bins] R1/R3 spectral accumulators (re, im per bin; spec_step)
    unsigned long long* stats;  // [KURA_NSTATS] (kura.h)
    unsigned long long* stamps; // [NWAVES][KURA_NSTAMP] phase cycle counters (KURA_STAMPS builds only)
    // split groups (N > 1024): npart workgroups share an env group, each owns
    // N/npart oscillators (a part: 256, 512 or 1024, KuraConfig.part_osc);
    // they exchange sin/cos images and partial sums through
    // global memory with agent-scope release/acquire (group_barrier).
    int npart;              // workgroups per env group (1 when N <= 1024)
    int npairs;             // env groups x npart
    float* xg;              // [group][2][npart][xl_img(part/256)] sin/cos images
    float* xred;            // [group][2][npart][RC][16] f32 partial sums
    double* xredd;          // [group][2][npart][RC][16] f64 partial sums
    unsigned* gcnt;         // [group][16] arrival counters, zeroed before every launch
    // episode true-LFP record (cfg.episode_cap > 0): kura_episode_bbpow
    int episode_cap;
    float* ep_lfp;          // [B][episode_cap] theta_mean samples of the running episode
    int* ep_len;            // [B] samples appended since the env's last reset
    int* eflags;            // [B] per-env failure bits of the last launch (KURA_F_*, kura.h), 0 = ok
    float* rows;            // optional [B][KURA_S_MAX+1][N]: every saved row of a step (sol_state_, env.py:430,440)
    double* lfp_tr;         // optional [B][n_transient - 1]: the LFP of every transient row of a reset but the
                            // last (theta_record_transient, env.py:611); NULL: only the last W rows are evaluated
    float* rows_tr;         // optional [B][n_transient][N]: every row of a reset's transient (sol_state after
                            // reset(), env.py:610); NULL: not kept
    int n_tr;               // rows per env of rows_tr (len(arange(0, transient_len, dt)))
    float* gemm_dump;       // KURA_DEBUG builds: [sweep][2][32][N] operand and coupling sums of workgroup 0
    int gemm_dump_n;        // ... sweeps to keep (kura_debug_gemm_dump)
};

// Device code reads DevParams where the dispatch put it: in the kernarg
// segment (constant address space, scalar loads).  Every kernel takes it by
// value as its FIRST argument (so it sits at kernarg offset 0) and reads it
// through kargs(); taking the by-value parameter's address instead makes the
// compiler copy the ~600-byte struct into every lane's scratch for the
// called solver to point at (K1 <4, false>: 1152 -> 560 B of scratch per
// lane, profiles/r04_resource_usage.txt; +0.8 % in the same-box A/B).
typedef const __attribute__((address_space(4))) DevParams DevParamsK;
__device__ __forceinline__ DevParamsK& kargs() {
    return *(DevParamsK*)__builtin_amdgcn_kernarg_segment_ptr();
}

// Diagnostic phase timers (compile with -DKURA_STAMPS): per wave, cycles
// spent in each phase (tools/phase_stamps.py names them), accumulated with
// s_memtime and added into p.stamps[wave][KURA_NSTAMP] at the end.
#define KURA_NSTAMP 24
#ifdef KURA_STAMPS
#define STAMP_DECL unsigned long long st_acc[KURA_NSTAMP] = {}; unsigned long long st_last = __builtin_amdgcn_s_memtime();
#define STAMP(k) do { unsigned long long n_ = __builtin_amdgcn_s_memtime(); st_acc[k] += n_ - st_last; st_last = n_; } while (0)
#define STAMP_FLUSH(p) do { if ((threadIdx.x & 63) == 0 && (p).stamps) for (int k_ = 0; k_ < KURA_NSTAMP; ++k_) atomicAdd(&(p).stamps[(threadIdx.x >> 6) * KURA_NSTAMP + k_], st_acc[k_]); } while (0)
#define STAMP_PARAMS , unsigned long long (&st_acc)[KURA_NSTAMP], unsigned long long& st_last
#define STAMP_ARGS , st_acc, st_last
#else
#define STAMP_DECL
#define STAMP(k) do { } while (0)
#define STAMP_FLUSH(p) do { } while (0)
#define STAMP_PARAMS
#define STAMP_ARGS
#endif

// Debug build (-DKURA_DEBUG, libkura_debug.so): every record, alpha, ring and
// LFP-sample access is checked against the extent of its buffer; a violation
// raises KURA_F_BOUNDS in kura_get_stats()[3] (and the per-env flags of the
// envs the launch finishes), so a raw buffer access that the hardware range
// check would silently turn into a zero read or a dropped store is named.
#ifdef KURA_DEBUG
#define KDBG_CHECK(stats, ok)                                                                     \
    do {                                                                                          \
        if ((stats) && !(ok)) atomicOr((stats) + 3, (unsigned long long)KURA_F_BOUNDS);           \
    } while (0)
#else
#define KDBG_CHECK(stats, ok) do { } while (0)
#endif

// Per-workgroup LDS besides the dynamic 32 x N operand: LFP samples of the
// current step (one row per env).
__shared__ float s_smp_n[E_WG][KURA_S_MAX + 2];
__shared__ double s_smp_r[E_WG][KURA_S_MAX + 2];

// LDS index of X[row][k] in MFMA A-fragment order: for k-block kb = k/8,
// lane (row + 32*(k&1)) holds its 4 consecutive k-steps in 16 contiguous
// bytes (one ds_read_b128).  Each 32-lane half is followed by a 16-byte pad
// (block = 264 floats), which makes the row-strided epilogue reads and the
// R64-layout stage-input writes bank-conflict free.
#define XS_HALF 132
#define XS_BLOCK 264
// split groups (N > 1024)
#define XL_NL 1024                       // default (largest) oscillators per part
#define XL_KC 512                        // oscillators per streamed GEMM chunk
#define XL_CIMG (XL_KC / 8 * XS_BLOCK)   // floats of one chunk image
#define XL_SPIN_MAX (1u << 25)
// alpha ring depth (k-blocks) of the split-group GEMM at TPW = 1 / 2 / 4
constexpr int KURA_XL_DEPTH1 = 8, KURA_XL_DEPTH2 = 8, KURA_XL_DEPTH4 = 4;
// split groups in BF16X3: parts of up to KURA_XL_SP_STAGED_MAXTPW * 256
// oscillators stage the split operand and split alpha in registers
// (coupling_gemm_xl_bf16x3); larger parts split per k-block with pre-split,
// deduplicated alpha (coupling_gemm_xl_bf16x3_kb); same-box A/B,
// profiles/r05_dedup_and_xl_forms_ab.txt
constexpr int KURA_XL_SP_STAGED_MAXTPW = 1;
// ... and the alpha ring of the bf16x3 forms, in 16-deep k-blocks (12 VGPRs per tile each)
constexpr int KURA_XL_SP_DEPTH1 = 8, KURA_XL_SP_DEPTH2 = 4, KURA_XL_SP_DEPTH4 = 2;
__host__ __device__ constexpr int xs_floats(int N) { return (N / 8) * XS_BLOCK; }
// floats of one part's LDS / global sin/cos image (TPW column tiles per wave)
__host__ __device__ constexpr int xl_img(int tpw) { return xs_floats(tpw * 256); }
__device__ __forceinline__ int xs_idx(int row, int k) {
    return (k >> 3) * XS_BLOCK + (k & 1) * XS_HALF + (row << 2) + ((k >> 1) & 3);
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

struct Grid {
    double start, delta;
    int n;
};
// np.arange(start, stop, step) in float64 (oracle arange()).
__device__ __forceinline__ Grid make_grid(double start, double stop, double step) {
    Grid g;
    double len = ceil((stop - start) / step);
    g.n = len > 0.0 ? (int)len : 0;
    g.start = start;
    g.delta = (start + step) - start;
    return g;
}
__device__ __forceinline__ double grid_at(const Grid& g, int i) {
    return i == 0 ? g.start : g.start + (double)i * g.delta;
}

// ---------------------------------------------------------------- GEMM ----
// acc[t] (32 x 32 tile, columns jt = wave*TPW + t) = X (LDS) x B-fragments.
// alpha fragments are read as global (addrspace 1) 16-byte loads so the
// compiler can count vmcnt precisely; two buffers give a prefetch distance of
// one k-block (16 MFMAs of this wave + the partner wave's) per load.
typedef const __attribute__((address_space(1))) floatx4 gfloatx4;
typedef __attribute__((address_space(1))) floatx4 gfx4;
typedef __attribute__((address_space(1))) float gfloat;

// Wave-uniform copy of a pointer (SGPRs): pointers read through the solver's
// VGPR-passed DevParams reference would otherwise stay per-lane (flat
// addressing, 64-bit VALU address math, spills).
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* ptr) {
    const uint64_t v = (uint64_t)(uintptr_t)ptr;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (T*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}


// KURA_COUPLING_BF16X3 (kura.h): the coupling from
// three-way bf16 splits on v_mfma_f32_32x32x16_bf16, six part products per
// 16-deep k-block in the order x1a1, x1a2, x2a1, x1a3, x2a2, x3a1 (the oracle
// restates the MFMA's accumulation exactly: oracle_split_gemm_rows, pinned by
// tests/test_mfma_bf16_model.py and the bitwise GEMM tests of
// tests/test_gpu_parity.py).  alpha
// arrives pre-split (split_alpha, kura_capi.inc): per column tile jt, k-block
// b and part p, lane l holds 8 bf16 at k = 16b + 8(i/4) + 2(i%4) + l/32 -- the
// k order of the fp32 operand image, so the sin/cos rows are split from the
// same two float4 reads of the LDS operand.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// Pairwise: one v_cvt_pk_bf16_f32 (round to nearest even) per two values and
// part, the bf16 pair widened back by a shift and a mask, the residual by one
// v_pk_add_f32 -- 9 VALU per pair.  The same values as converting element by
// element (each residual x - bf16(x) is exact in fp32).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned pk_bf16(f32x2 x) { return __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2)); }
__device__ __forceinline__ f32x2 unpk_bf16(unsigned u) {
    return f32x2{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
}
__device__ __forceinline__ void split_bf16x3(floatx4 lo, floatx4 hi, bf16x8& h1, bf16x8& h2, bf16x8& h3) {
    u32x4 a, b, c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x2 x = q < 2 ? f32x2{lo[2 * q], lo[2 * q + 1]} : f32x2{hi[2 * q - 4], hi[2 * q - 3]};
        const unsigned ua = pk_bf16(x);
        const f32x2 r1 = x - unpk_bf16(ua);
        const unsigned ub = pk_bf16(r1);
        const f32x2 r2 = r1 - unpk_bf16(ub);
        a[q] = ua;
        b[q] = ub;
        c[q] = pk_bf16(r2);
    }
    h1 = __builtin_bit_cast(bf16x8, a);
    h2 = __builtin_bit_cast(bf16x8, b);
    h3 = __builtin_bit_cast(bf16x8, c);
}

// One 16-deep k-block of a BF16X3 tile: the six part products in the order of
// the oracle's oracle_split_gemm_rows (x1a1, x1a2, x2a1, x1a3, x2a2, x3a1).
// The order is the numerics contract (the MFMA's accumulation is not
// associative); every BF16X3 GEMM body below states it through this helper.
__device__ __forceinline__ void mfma6_bf16x3(bf16x8 x1, bf16x8 x2, bf16x8 x3, bf16x8 a1, bf16x8 a2, bf16x8 a3,
                                             floatx16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1, a1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1, a2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2, a1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1, a3, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2, a2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3, a1, acc, 0, 0, 0);
}

template <int TPW>
__device__ __forceinline__ void coupling_gemm_bf16x3(const float* __restrict__ Xs, const float* __restrict__ alpha_sw,
                                                     floatx16 (&acc)[TPW], unsigned long long* dbg = nullptr) {
    (void)dbg;
    constexpr int N = TPW * 32 * NWAVES;
    constexpr int NB = N / 16;
    constexpr int TSTRIDE = NB * 3 * 64 * 16;   // bytes per column tile
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const floatx4* xs4 = reinterpret_cast<const floatx4*>(Xs + (lane >> 5) * XS_HALF + (lane & 31) * 4);
    const float* au = uniform_ptr(alpha_sw);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)au + (size_t)wave * TPW * TSTRIDE), 0, TPW * TSTRIDE, 0x00020000);
    auto ld = [&](int t, int b, int p) -> bf16x8 {
        KDBG_CHECK(dbg, b >= 0 && b < NB && ((b * 3 + p) * 64 + lane) * 16 + t * TSTRIDE + 16 <= TPW * TSTRIDE);
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, ((b * 3 + p) * 64 + lane) * 16,
                                                                                 t * TSTRIDE, 0));
    };
    // two register sets per tile: block b+2's parts load right after block
    // b's MFMAs, a whole block of cover (one set: the loads issue after the
    // block's last x3*a1 and the next block's first MFMA waits on them;
    // +2 % on the step, profiles/r05_k1_ring2_ab.txt)
    bf16x8 a1[2][TPW], a2[2][TPW], a3[2][TPW];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            a1[d][t] = ld(t, d < NB ? d : NB - 1, 0);
            a2[d][t] = ld(t, d < NB ? d : NB - 1, 1);
            a3[d][t] = ld(t, d < NB ? d : NB - 1, 2);
        }
    auto blk = [&](int b, int d) __attribute__((always_inline)) {
        bf16x8 x1, x2, x3;
        split_bf16x3(xs4[(2 * b) * (XS_BLOCK / 4)], xs4[(2 * b + 1) * (XS_BLOCK / 4)], x1, x2, x3);
        const int bn = b + 2 < NB ? b + 2 : NB - 1;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            mfma6_bf16x3(x1, x2, x3, a1[d][t], a2[d][t], a3[d][t], acc[t]);
            a1[d][t] = ld(t, bn, 0);
            a2[d][t] = ld(t, bn, 1);
            a3[d][t] = ld(t, bn, 2);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    static_assert(NB % 2 == 0, "two-block ring");
#pragma unroll 1
    for (int b = 0; b < NB; b += 2) {
        blk(b, 0);
        blk(b + 1, 1);
    }
}

// The same GEMM at TPW = 4 (N = 1024) for an alpha with the grid's shift
// structure (alpha_shift_reuse, kura_capi.inc; DevParams.alpha_reuse):
//   fragment(jt, b) == fragment(jt - 1, b - 2)   for jt % 4 != 0 and b % 8 >= 2,
// which every alpha = f(grid distance) on the 16 x 8 x 8 grid has -- a wave's
// four tiles are four x-lines each of one z-plane, a k-block b = 8 zk + xb is
// x-lines 2xb, 2xb+1 of plane zk, so a fragment depends on |z_wave - zk| and
// on the displacement d = xb - 2t alone.  Within a group of 8 k-blocks (one
// zk) d takes 14 values, and at any block the live ones are 8 consecutive:
// the fragment of displacement d lives in physical set (d + 6) mod 8, named
// statically (the 8 blocks fully unrolled), and tile t at block xb reads set
// (xb - 2t + 6) mod 8 -- what tile t-1 read two blocks earlier.  Loaded are
// only tile 0's fragments and blocks 0, 1 of a group: 14 sets per group
// instead of 32 (360 loads per sweep instead of the two-block ring's 792,
// both counting their clamped, unused tail prefetch), no moves, no LDS, no
// scalar loads, the same 96 VGPRs as the two-block ring.
//   after block xb < 6: tile 3's set (xb) has died, it takes tile 0's
//     fragment of block xb + 2 (d = xb + 2, the same set);
//   after blocks 6, 7: all four sets have died; tile t's takes tile t+1's
//     (mod 4) fragment of the next group's block xb - 6.
// The tiles of a block run 3, 2, 1, 0: the mid-group refill issues first and
// is read last, two blocks later.  Per tile the k-blocks ascend and each is
// the six products in the oracle's order, so every acc[t] sees the sequence
// of coupling_gemm_bf16x3 and the sums are bit-identical.
__device__ __forceinline__ void coupling_gemm_bf16x3_shift(const float* __restrict__ Xs,
                                                           const float* __restrict__ alpha_sw, floatx16 (&acc)[4],
                                                           unsigned long long* dbg = nullptr) {
    (void)dbg;
    constexpr int TPW = 4;
    constexpr int N = TPW * 32 * NWAVES;
    constexpr int NB = N / 16;
    constexpr int GB = 8;                       // k-blocks per group (one z-plane of the operand)
    constexpr int TSTRIDE = NB * 3 * 64 * 16;   // bytes per column tile
    static_assert(NB % GB == 0, "whole groups");
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const floatx4* xs4 = reinterpret_cast<const floatx4*>(Xs + (lane >> 5) * XS_HALF + (lane & 31) * 4);
    const float* au = uniform_ptr(alpha_sw);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)au + (size_t)wave * TPW * TSTRIDE), 0, TPW * TSTRIDE, 0x00020000);
    auto ld = [&](int t, int b, int p) -> bf16x8 {
        KDBG_CHECK(dbg, t >= 0 && t < TPW && b >= 0 && b < NB &&
                            ((b * 3 + p) * 64 + lane) * 16 + t * TSTRIDE + 16 <= TPW * TSTRIDE);
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, ((b * 3 + p) * 64 + lane) * 16,
                                                                                 t * TSTRIDE, 0));
    };
    bf16x8 a1[GB], a2[GB], a3[GB];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int s = (d - 2 * t + 6) & 7;
            a1[s] = ld(t, d, 0);
            a2[s] = ld(t, d, 1);
            a3[s] = ld(t, d, 2);
        }
#pragma unroll 1
    for (int b0 = 0; b0 < NB; b0 += GB) {
#pragma unroll
        for (int xb = 0; xb < GB; ++xb) {
            bf16x8 x1, x2, x3;
            split_bf16x3(xs4[(2 * (b0 + xb)) * (XS_BLOCK / 4)], xs4[(2 * (b0 + xb) + 1) * (XS_BLOCK / 4)], x1, x2, x3);
#pragma unroll
            for (int t = TPW - 1; t >= 0; --t) {
                const int s = (xb - 2 * t + 6) & 7;
                mfma6_bf16x3(x1, x2, x3, a1[s], a2[s], a3[s], acc[t]);
                if (xb < GB - 2) {
                    if (t == TPW - 1) {   // the one set that died: tile 0's fragment of block xb + 2
                        a1[s] = ld(0, b0 + xb + 2, 0);
                        a2[s] = ld(0, b0 + xb + 2, 1);
                        a3[s] = ld(0, b0 + xb + 2, 2);
                    }
                } else {   // the next group's blocks 0, 1
                    // (the last group loads its own again, unused: a branch
                    // around these loads makes the waits of blocks 6, 7 cover
                    // the path without them -- vmcnt(0..2), which drains the
                    // prefetch on every other group)
                    const int tn = (t + 1) & 3, bn = (b0 + GB < NB ? b0 + GB : b0) + xb - (GB - 2);
                    a1[s] = ld(tn, bn, 0);
                    a2[s] = ld(tn, bn, 1);
                    a3[s] = ld(tn, bn, 2);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// KURA_COUPLING_F32: exact fp32, the k-ordered fmaf chain of
// v_mfma_f32_32x32x2_f32.  Wave w owns column tiles w*TPW .. w*TPW+TPW-1.
template <int TPW>
__device__ __forceinline__ void coupling_gemm_f32(const float* __restrict__ Xs, const float* __restrict__ alpha_sw,
                                                  floatx16 (&acc)[TPW], unsigned long long* dbg = nullptr) {
    (void)dbg;  // KURA_DEBUG: bounds flag target
    constexpr int N = TPW * 32 * NWAVES;
    constexpr int NK8 = N / 8;
    constexpr int TSTRIDE = NK8 * 64;  // floatx4 per column tile
    // lane id re-derived here (volatile: never CSE'd with a long-lived value),
    // so the loop's addresses are not reloaded from a spill slot in the
    // preheader -- such a reload makes the loop-header wait vmcnt(0), which
    // would drain the alpha prefetch every iteration.
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    // lane l reads floats [kb*XS_BLOCK + (l>>5)*XS_HALF + (l&31)*4, +4)
    const floatx4* xs4 = reinterpret_cast<const floatx4*>(Xs + (lane >> 5) * XS_HALF + (lane & 31) * 4);
    // alpha via raw buffer loads: wave-uniform descriptor (this wave's TPW
    // column tiles), 32-bit lane offset, tile offset in an SGPR -- no 64-bit
    // address VALU between the MFMAs (isolated: 150 vs 130 TFLOP/s with
    // global_load, tools/gemm_bench.hip).  Two register buffers, one k-block
    // of cover; sched_barrier keeps each refill right after the MFMAs that
    // consumed the buffer (the scheduler would sink them to the loop end).
    // Loads past the last k-block are clamped so the count per iteration is
    // fixed (exact vmcnt).
    // (the descriptor must be provably wave-uniform, else every load becomes a
    // readfirstlane waterfall loop: alpha_sw reaches this non-inlined solver
    // through a VGPR-passed reference, so force it into SGPRs)
    const float* au = uniform_ptr(alpha_sw);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(au + (size_t)wave * TPW * TSTRIDE * 4), 0, TPW * TSTRIDE * 16, 0x00020000);
    auto ld = [&](int t, int k) -> floatx4 {
        KDBG_CHECK(dbg, k >= 0 && k < NK8 && (lane + k * 64) * 16 + t * TSTRIDE * 16 + 16 <=
                                                                        TPW * TSTRIDE * 16);
        return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rs, (lane + k * 64) * 16,
                                                                                 t * TSTRIDE * 16, 0));
    };
    floatx4 b0[TPW], b1[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        b0[t] = ld(t, 0);
        b1[t] = ld(t, 1);
    }
#pragma unroll 1
    for (int kb = 0; kb < NK8; kb += 2) {
        floatx4 a = xs4[kb * (XS_BLOCK / 4)];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0[t][s], acc[t], 0, 0, 0);
        const int k2 = kb + 2 < NK8 ? kb + 2 : NK8 - 1;
#pragma unroll
        for (int t = 0; t < TPW; ++t) b0[t] = ld(t, k2);
        __builtin_amdgcn_sched_barrier(0);
        a = xs4[(kb + 1) * (XS_BLOCK / 4)];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1[t][s], acc[t], 0, 0, 0);
        const int k3 = kb + 3 < NK8 ? kb + 3 : NK8 - 1;
#pragma unroll
        for (int t = 0; t < TPW; ++t) b1[t] = ld(t, k3);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// K1's BF16X3 GEMM reading alpha through the deduplicated image (the
// split-group image: a map [NB][N/32] of int32 byte offsets, then the
// distinct B fragments; 112 of 2048 at N = 1024, 336 KB -- always L2
// resident).  Same fragments, same MFMAs in the same order as
// coupling_gemm_bf16x3, so the sums are identical; the fragment offsets are
// scalar loads one k-block ahead of the refill they serve.  Used by the
// reset (solve_wg): over its ~457 sweeps the workgroups of an XCD drift apart
// and the 6 MiB streamed image misses L2; warm B=4096 env0
// reset 56.3 -> 53.3 ms, same box (profiles/r06_reset_dedup_ab.txt).  The
// step keeps the streamed image: the scalar-loaded map cost it 7 %.
template <int TPW>
__device__ __forceinline__ void coupling_gemm_bf16x3_dd(const float* __restrict__ Xs, const float* __restrict__ alpha_dd,
                                                        unsigned img_bytes, floatx16 (&acc)[TPW]) {
    constexpr int N = TPW * 32 * NWAVES;
    constexpr int NB = N / 16, NT = N / 32;
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const floatx4* xs4 = reinterpret_cast<const floatx4*>(Xs + (lane >> 5) * XS_HALF + (lane & 31) * 4);
    const float* au = uniform_ptr(alpha_dd);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)au, 0, __builtin_amdgcn_readfirstlane(img_bytes), 0x00020000);   // map + distinct fragments
    // the map through the constant address space: scalar loads (s_load_dword)
    typedef const __attribute__((address_space(4))) int cint;
    cint* mp = reinterpret_cast<cint*>(reinterpret_cast<uintptr_t>(au)) + wave * TPW;   // map row b: mp[b * NT + t]
    auto off = [&](int t, int b) -> int { return mp[b * NT + t]; };
    auto ld = [&](int o, int p) -> bf16x8 {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (p * 64 + lane) * 16, o, 0));
    };
    bf16x8 a1[2][TPW], a2[2][TPW], a3[2][TPW];
    int om[TPW];   // offsets of block b+2 (the next refill)
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int o = off(t, d);
            a1[d][t] = ld(o, 0);
            a2[d][t] = ld(o, 1);
            a3[d][t] = ld(o, 2);
        }
#pragma unroll
    for (int t = 0; t < TPW; ++t) om[t] = off(t, 2 < NB ? 2 : NB - 1);
    auto blk = [&](int b, int d) __attribute__((always_inline)) {
        bf16x8 x1, x2, x3;
        split_bf16x3(xs4[(2 * b) * (XS_BLOCK / 4)], xs4[(2 * b + 1) * (XS_BLOCK / 4)], x1, x2, x3);
        const int bn3 = b + 3 < NB ? b + 3 : NB - 1;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            mfma6_bf16x3(x1, x2, x3, a1[d][t], a2[d][t], a3[d][t], acc[t]);
            const int o = om[t];
            a1[d][t] = ld(o, 0);
            a2[d][t] = ld(o, 1);
            a3[d][t] = ld(o, 2);
            om[t] = off(t, bn3);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    static_assert(NB % 2 == 0, "two-block ring");
#pragma unroll 1
    for (int b = 0; b < NB; b += 2) {
        blk(b, 0);
        blk(b + 1, 1);
    }
}

// The coupling GEMM of a handle's arithmetic (SP: KURA_COUPLING_BF16X3).
// reuse (DevParams.alpha_reuse, decided by the host from the data): alpha has
// the shift structure, BF16X3 at TPW = 4 takes coupling_gemm_bf16x3_shift.
template <int TPW, bool SP>
__device__ __forceinline__ void coupling_gemm(const float* __restrict__ Xs, const float* __restrict__ alpha_sw,
                                              int reuse, floatx16 (&acc)[TPW], unsigned long long* dbg = nullptr) {
    if constexpr (SP) {
        if constexpr (TPW == 4) {
            if (__builtin_amdgcn_readfirstlane(reuse)) {   // wave-uniform: a scalar branch
                coupling_gemm_bf16x3_shift(Xs, alpha_sw, acc, dbg);
                return;
            }
        }
        coupling_gemm_bf16x3<TPW>(Xs, alpha_sw, acc, dbg);
    } else
        coupling_gemm_f32<TPW>(Xs, alpha_sw, acc, dbg);
}

// Workgroup barrier that orders LDS only.  Inside a solve every workspace
// record (R) is written and read back by the same lane (MFMA-layout
// ownership), so the release half of __syncthreads -- which also drains every
// outstanding global store and load (vmcnt(0)) -- is not needed there; only
// LDS (the GEMM operand, control slots, reduction partials) is shared.
__device__ __forceinline__ void lds_barrier() {
    // compiler-only barrier for the records (buffer loads/stores through the
    // workgroup's descriptor): nothing may be reordered across a phase boundary
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    asm volatile("" ::: "memory");
}

// Split-group GEMM (N > 1024): the same MFMA chain over all N oscillators
// (k ascending, so P/Q are bit-identical to coupling_gemm's), with the
// 32 x N sin/cos operand streamed from the group's global image (xg) through
// two LDS chunk buffers of XL_KC oscillators, and this workgroup's TPW*256 output
// columns (col0 ..) of alpha.
template <int TPW>
__device__ __forceinline__ void coupling_gemm_xl(const float* __restrict__ xg, const float* __restrict__ alpha_sw,
                                                 float* Xs, int NG, int col0, floatx16 (&acc)[TPW] STAMP_PARAMS) {
    // (xg, NG, col0 arrive through the VGPR-passed Part of the non-inlined
    // solver; they are wave-uniform, readfirstlane makes that provable)
    NG = __builtin_amdgcn_readfirstlane(NG);  // all addressing below must be provably uniform
    col0 = __builtin_amdgcn_readfirstlane(col0);
    xg = uniform_ptr(xg);
    const int NK8 = NG / 8;
    const int TSTRIDE = NK8 * 64;  // floatx4 per column tile
    const int nchunk = NG / XL_KC;
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const float* au = uniform_ptr(alpha_sw);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(au + ((size_t)(col0 / 32) + wave * TPW) * TSTRIDE * 4), 0, TPW * TSTRIDE * 16, 0x00020000);
    auto ld = [&](int t, int k) -> floatx4 {
        return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rs, (lane + k * 64) * 16,
                                                                                 t * TSTRIDE * 16, 0));
    };
    // chunk 0 -> LDS buffer 0
    constexpr int C4 = XL_CIMG / 4;               // floatx4 per chunk image
    constexpr int CPT = (C4 + NTHREADS - 1) / NTHREADS;
    gfloatx4* xg4 = (gfloatx4*)xg;
    floatx4* xs4w = (floatx4*)Xs;
    for (int k = threadIdx.x; k < C4; k += NTHREADS) xs4w[k] = xg4[k];
    lds_barrier();
    STAMP(18);  // split groups: chunk 0 staged (slot 18 is free outside KURA_STAMPS_SI)
    // alpha ring of XD k-blocks per tile: the load of k-block kb + XD is
    // issued right after the MFMAs of kb, so it has XD - 1 k-blocks of this
    // wave's and its SIMD partner's MFMAs to arrive.  With TPW = 4 a k-block is
    // 16 MFMAs per wave and XD = 2 covers the L2 latency; at TPW = 1 (parts of
    // 256) a k-block is only 4 MFMAs, and a ring of 2 left the MFMAs waiting on
    // alpha (DESIGN.md section 5, K1').  The ring costs XD * TPW * 4 VGPRs.
    constexpr int XD = TPW >= 4 ? KURA_XL_DEPTH4 : (TPW == 2 ? KURA_XL_DEPTH2 : KURA_XL_DEPTH1);
    constexpr int KPC = XL_KC / 8;                 // k-blocks per chunk
    constexpr int PRE = (CPT + XD - 1) / XD * XD;  // unrolled head: one staging load per k-block
    static_assert(KPC % XD == 0 && PRE <= KPC, "alpha ring must tile the chunk");
    floatx4 bq[XD][TPW];
#pragma unroll
    for (int d = 0; d < XD; ++d)
#pragma unroll
        for (int t = 0; t < TPW; ++t) bq[d][t] = ld(t, d);
    // k-block kb (local) of the chunk whose LDS image is xs4, ring slot d = kb % XD;
    // the A fragment of the next k-block is read from LDS one block ahead
    floatx4 an;
    auto kblock = [&](const floatx4* xs4, int kg0, int kb, int d) __attribute__((always_inline)) {
        const floatx4 a = an;
        an = xs4[(kb + 1 < KPC ? kb + 1 : KPC - 1) * (XS_BLOCK / 4)];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < TPW; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bq[d][t][s], acc[t], 0, 0, 0);
        const int kn = kg0 + kb + XD < NK8 ? kg0 + kb + XD : NK8 - 1;
#pragma unroll
        for (int t = 0; t < TPW; ++t) bq[d][t] = ld(t, kn);
    };
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        const floatx4* xs4 = reinterpret_cast<const floatx4*>(Xs + (c & 1) * XL_CIMG + (lane >> 5) * XS_HALF +
                                                              (lane & 31) * 4);
        const int kg0 = c * KPC;
        const bool more = c + 1 < nchunk;
        an = xs4[0];
        // the next chunk is staged in registers one float4 per k-block, each
        // load issued right after that block's alpha loads, so the in-order
        // vmcnt waits of later blocks cover it without a stall
        floatx4 nx[CPT];
#pragma unroll
        for (int kb = 0; kb < PRE; ++kb) {
            kblock(xs4, kg0, kb, kb % XD);
            const int k = threadIdx.x + kb * NTHREADS;
            if (kb < CPT && more && k < C4) nx[kb] = xg4[(size_t)(c + 1) * C4 + k];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll 1
        for (int kb = PRE; kb < KPC; kb += XD) {
#pragma unroll
            for (int d = 0; d < XD; ++d) {
                kblock(xs4, kg0, kb + d, d);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (more) {  // the other buffer was last read in chunk c-1, before the previous barrier
            floatx4* dst = (floatx4*)(Xs + ((c + 1) & 1) * XL_CIMG);
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
                const int k = threadIdx.x + u * NTHREADS;
                if (k < C4) dst[k] = nx[u];
            }
        }
        STAMP(2);
        lds_barrier();
        STAMP(17);  // split groups: chunk barrier wait (slot 17 is free outside KURA_STAMPS_SI)
    }
}


// The split-group BF16X3 GEMM for parts of 512 and 1024 (TPW = 2, 4): the
// sin/cos operand streamed in fp32 chunks of 512 as in coupling_gemm_xl and
// split per k-block in every wave (shared by the wave's tiles), the
// pre-split alpha fragments through a ring of XD 16-deep k-blocks per tile,
// each fragment found through the image's offset map (the offsets of the
// next refill read one k-block ahead).  At TPW >= 2 this beats the staged
// split below (its chunks of 256 double the chunk barriers; same-box A/B,
// profiles/r05_dedup_and_xl_forms_ab.txt).
template <int TPW>
__device__ __forceinline__ void coupling_gemm_xl_bf16x3_kb(const float* __restrict__ xg, const float* __restrict__ alpha_sw,
                                                        float* Xs, int NG, int col0, floatx16 (&acc)[TPW],
                                                        unsigned long long* dbg STAMP_PARAMS) {
    (void)dbg;
    NG = __builtin_amdgcn_readfirstlane(NG);
    col0 = __builtin_amdgcn_readfirstlane(col0);
    xg = uniform_ptr(xg);
    const int NB = NG / 16;
    const int NT = NG / 32;
    constexpr int FRAG = 3 * 64 * 16;      // bytes per B fragment
    const int nchunk = NG / XL_KC;
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const float* au = uniform_ptr(alpha_sw);
    // the deduplicated image (split_alpha_dedup: a map [NB][NT] of byte
    // offsets, then the distinct fragments): at N = 8192 the 131072
    // fragments of the reference's alpha are 992 distinct ones (3 MB)
    const unsigned IMG = (unsigned)NT * NB * 4u + (unsigned)NT * NB * FRAG;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)au, 0, IMG, 0x00020000);
    const float* mp = au + col0 / 32 + wave * TPW;          // map row b: mp[b * NT + t]
    auto off = [&](int t, int b) -> int { return __builtin_bit_cast(int, mp[(size_t)b * NT + t]); };
    auto ld = [&](int o, int p) -> bf16x8 {
        KDBG_CHECK(dbg, o >= NT * NB * 4 && (unsigned)o + FRAG <= IMG);
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (p * 64 + lane) * 16, o, 0));
    };
    constexpr int C4 = XL_CIMG / 4;
    constexpr int CPT = (C4 + NTHREADS - 1) / NTHREADS;
    gfloatx4* xg4 = (gfloatx4*)xg;
    floatx4* xs4w = (floatx4*)Xs;
    for (int k = threadIdx.x; k < C4; k += NTHREADS) xs4w[k] = xg4[k];
    lds_barrier();
    STAMP(18);
    constexpr int XD = TPW >= 4 ? KURA_XL_SP_DEPTH4 : (TPW == 2 ? KURA_XL_SP_DEPTH2 : KURA_XL_SP_DEPTH1);
    constexpr int KPC = XL_KC / 16;                // 16-deep k-blocks per chunk
    constexpr int PRE = (CPT + XD - 1) / XD * XD;
    static_assert(KPC % XD == 0 && PRE <= KPC, "alpha ring must tile the chunk");
    bf16x8 q1[XD][TPW], q2[XD][TPW], q3[XD][TPW];
    int om[TPW];   // fragment offsets of the next ring refill's k-block
#pragma unroll
    for (int d = 0; d < XD; ++d)
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int o = off(t, d);
            q1[d][t] = ld(o, 0);
            q2[d][t] = ld(o, 1);
            q3[d][t] = ld(o, 2);
        }
#pragma unroll
    for (int t = 0; t < TPW; ++t) om[t] = off(t, XD < NB ? XD : NB - 1);
    floatx4 an0, an1;   // the next k-block's two float4 of the operand (LDS, one block ahead)
    auto kblock = [&](const floatx4* xs4, int kg0, int kb, int d) __attribute__((always_inline)) {
        const floatx4 lo = an0, hi = an1;
        const int nb = kb + 1 < KPC ? kb + 1 : KPC - 1;
        an0 = xs4[(2 * nb) * (XS_BLOCK / 4)];
        an1 = xs4[(2 * nb + 1) * (XS_BLOCK / 4)];
        bf16x8 x1, x2, x3;
        split_bf16x3(lo, hi, x1, x2, x3);
#pragma unroll
        for (int t = 0; t < TPW; ++t) mfma6_bf16x3(x1, x2, x3, q1[d][t], q2[d][t], q3[d][t], acc[t]);
        const int kn1 = kg0 + kb + XD + 1 < NB ? kg0 + kb + XD + 1 : NB - 1;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int o = om[t];
            q1[d][t] = ld(o, 0);
            q2[d][t] = ld(o, 1);
            q3[d][t] = ld(o, 2);
            om[t] = off(t, kn1);
        }
    };
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        const floatx4* xs4 = reinterpret_cast<const floatx4*>(Xs + (c & 1) * XL_CIMG + (lane >> 5) * XS_HALF +
                                                              (lane & 31) * 4);
        const int kg0 = c * KPC;
        const bool more = c + 1 < nchunk;
        an0 = xs4[0];
        an1 = xs4[XS_BLOCK / 4];
        floatx4 nx[CPT];
#pragma unroll
        for (int kb = 0; kb < PRE; ++kb) {
            kblock(xs4, kg0, kb, kb % XD);
            const int k = threadIdx.x + kb * NTHREADS;
            if (kb < CPT && more && k < C4) nx[kb] = xg4[(size_t)(c + 1) * C4 + k];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll 1
        for (int kb = PRE; kb < KPC; kb += XD) {
#pragma unroll
            for (int d = 0; d < XD; ++d) {
                kblock(xs4, kg0, kb + d, d);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (more) {
            floatx4* dst = (floatx4*)(Xs + ((c + 1) & 1) * XL_CIMG);
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
                const int k = threadIdx.x + u * NTHREADS;
                if (k < C4) dst[k] = nx[u];
            }
        }
        STAMP(2);
        lds_barrier();
        STAMP(17);
    }
}

// The split-group GEMM in KURA_COUPLING_BF16X3 for parts of 256 (TPW = 1):
// coupling_gemm_bf16x3's chain (six part products per 16-deep k-block, k
// ascending over all NG oscillators, so P/Q are the oracle's
// oracle_split_gemm_rows at any N).  alpha comes from the fp32 image
// (swizzle_alpha) through a ring of XD k-blocks per tile and is split in
// registers (4 bytes per element instead of 6: at one tile per wave the
// CU's alpha fill rate, not VALU, bounds the loop).  The
// sin/cos operand is split ONCE per chunk, while it is staged: each thread
// loads the two float4 of (k-block, lane) pairs from the group image and
// writes their three bf16 parts to LDS, so the k-block loop reads x1/x2/x3
// with three ds_read_b128 (splitting per k-block in every wave was 8x
// redundant and made the TPW = 1 loop VALU-bound: ~57 VALU per 6 MFMAs).
// Chunks are XL_KC_SP oscillators (two split buffers of 48 KB).
#define XL_KC_SP 256
template <int TPW>
__device__ __forceinline__ void coupling_gemm_xl_bf16x3(const float* __restrict__ xg, const float* __restrict__ alpha_sw,
                                                        float* Xs, int NG, int col0, floatx16 (&acc)[TPW],
                                                        unsigned long long* dbg STAMP_PARAMS) {
    (void)dbg;
    NG = __builtin_amdgcn_readfirstlane(NG);
    col0 = __builtin_amdgcn_readfirstlane(col0);
    xg = uniform_ptr(xg);
    const int NB = NG / 16;
    const int TSTRIDE = NB * 2 * 64 * 16;   // bytes per column tile (the fp32 image)
    constexpr int KC = XL_KC_SP;
    constexpr int NBC = KC / 16;            // k-blocks per chunk
    constexpr int CB = NBC * 3 * 64;        // bf16x8 per chunk buffer
    constexpr int PAIRS = NBC * 64;         // (k-block, lane) pairs per chunk
    constexpr int PPT = PAIRS / NTHREADS;
    static_assert(PAIRS % NTHREADS == 0 && 2 * CB * 16 <= 2 * XL_CIMG * 4, "split chunks must fit the XL LDS");
    const int nchunk = NG / KC;
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const float* au = uniform_ptr(alpha_sw);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)au + ((size_t)(col0 / 32) + wave * TPW) * TSTRIDE), 0, TPW * TSTRIDE, 0x00020000);
    auto ldf = [&](int t, int k) -> floatx4 {   // k8-block k of the fp32 image
        KDBG_CHECK(dbg, k >= 0 && k < 2 * NB && (lane + k * 64) * 16 + t * TSTRIDE + 16 <= TPW * TSTRIDE);
        return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rs, (lane + k * 64) * 16,
                                                                                 t * TSTRIDE, 0));
    };
    gfloatx4* xg4 = (gfloatx4*)xg;
    bf16x8* xsb = reinterpret_cast<bf16x8*>(Xs);
    // the f32 float4 of pair pr (k-block pr/64 of chunk c, lane pr%64), half h
    // (k8-block 2b + h): the XS layout of the group image
    auto src = [&](int c, int pr, int h) -> size_t {
        const int b = pr >> 6, l = pr & 63;
        return ((size_t)c * (KC / 8) + 2 * b + h) * (XS_BLOCK / 4) + (l >> 5) * (XS_HALF / 4) + (l & 31);
    };
    auto put = [&](int buf, int pr, floatx4 lo, floatx4 hi) {
        bf16x8 x1, x2, x3;
        split_bf16x3(lo, hi, x1, x2, x3);
        const int b = pr >> 6, l = pr & 63;
        bf16x8* d = xsb + buf * CB + b * 3 * 64 + l;
        d[0] = x1;
        d[64] = x2;
        d[128] = x3;
    };
#pragma unroll
    for (int u = 0; u < PPT; ++u) {
        const int pr = threadIdx.x + u * NTHREADS;
        put(0, pr, xg4[src(0, pr, 0)], xg4[src(0, pr, 1)]);
    }
    lds_barrier();
    STAMP(18);
    constexpr int XD = TPW >= 4 ? KURA_XL_SP_DEPTH4 : (TPW == 2 ? KURA_XL_SP_DEPTH2 : KURA_XL_SP_DEPTH1);
    constexpr int NX = 2 * PPT;                    // staging loads per thread and chunk
    constexpr int PRE = (NX + XD - 1) / XD * XD;   // unrolled head: one staging load per k-block
    static_assert(NBC % XD == 0 && PRE <= NBC, "alpha ring must tile the chunk");
    floatx4 qlo[XD][TPW], qhi[XD][TPW];
#pragma unroll
    for (int d = 0; d < XD; ++d)
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            qlo[d][t] = ldf(t, 2 * d);
            qhi[d][t] = ldf(t, 2 * d + 1);
        }
    bf16x8 n1, n2, n3;   // the next k-block's operand parts (LDS, one block ahead)
    auto kblock = [&](const bf16x8* xb, int kg0, int kb, int d) __attribute__((always_inline)) {
        const bf16x8 x1 = n1, x2 = n2, x3 = n3;
        const int nb = kb + 1 < NBC ? kb + 1 : NBC - 1;
        n1 = xb[nb * 192];
        n2 = xb[nb * 192 + 64];
        n3 = xb[nb * 192 + 128];
        const int kn = kg0 + kb + XD < NB ? kg0 + kb + XD : NB - 1;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            bf16x8 a1, a2, a3;
            split_bf16x3(qlo[d][t], qhi[d][t], a1, a2, a3);
            qlo[d][t] = ldf(t, 2 * kn);
            qhi[d][t] = ldf(t, 2 * kn + 1);
            mfma6_bf16x3(x1, x2, x3, a1, a2, a3, acc[t]);
        }
    };
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        const bf16x8* xb = xsb + (c & 1) * CB + lane;
        const int kg0 = c * NBC;
        const bool more = c + 1 < nchunk;
        n1 = xb[0];
        n2 = xb[64];
        n3 = xb[128];
        floatx4 nx[NX];
#pragma unroll
        for (int kb = 0; kb < PRE; ++kb) {
            kblock(xb, kg0, kb, kb % XD);
            if (kb < NX && more) nx[kb] = xg4[src(c + 1, threadIdx.x + (kb >> 1) * NTHREADS, kb & 1)];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll 1
        for (int kb = PRE; kb < NBC; kb += XD) {
#pragma unroll
            for (int d = 0; d < XD; ++d) {
                kblock(xb, kg0, kb + d, d);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (more) {  // the other buffer was last read in chunk c-1, before the previous barrier
#pragma unroll
            for (int u = 0; u < PPT; ++u) put((c + 1) & 1, threadIdx.x + u * NTHREADS, nx[2 * u], nx[2 * u + 1]);
        }
        STAMP(2);
        lds_barrier();
        STAMP(17);
    }
}

// Per-env solver control.  One slot per local env lives in LDS; thread e
// (e < 16) owns slot e's scalar decisions, every lane reads it.
struct CtlE {
    double g_start, g_delta;  // save grid (np.arange start, (start+step)-start)
    int n;                    // grid length
    int si;                   // next save index
    int active;               // still integrating in this solve
    int nsteps, rejected, flags;
    int lfp_from, lfp_to, pos0;  // rows [from,to) feed LFP samples at pos0 + (si - from)
    int keep, nsave;          // decision of the last attempted step
    int acc_steps, acc_rej;   // over the solves of one launch (stats)
    float t1, tprev, tnext, h, dtn;
    // post_step decides and advances time in one section (before the saves
    // of the step): the save passes read the step's save index and
    // interval from here
    int sv_si;
    float sv_tprev, sv_tnext;
};
__shared__ CtlE s_ctl[E_WG];
__shared__ float s_kn[E_WG];  // per-env coupling gain of the workgroup's envs
#define RC 4     // save rounds per pass over the records: recorder (f64) LFP, split groups
#define RC_N 8   // ... naive LFP on one workgroup per env group (f32 partials only)
__shared__ float s_red[RC_N][NWAVES][E_WG];      // per-wave partial sums (f32)
__shared__ double s_redd[RC][NWAVES][E_WG];      // per-wave partial sums (f64, recorder LFP)
__shared__ float s_theta[E_WG][RC_N];            // dense-output abscissae of the rounds of a pass
__shared__ int s_rflag[E_WG][RC_N];              // bit0: save row, bit1: LFP row, bit2: final row
__shared__ double s_u[E_WG][4];                  // rescaled amplitudes (env.py:389-393)
__shared__ int s_nI[E_WG], s_nII[E_WG];          // ON / OFF grid lengths of the step (step_pair)

__device__ __forceinline__ double grid_at_c(const CtlE& c, int i) {
    return i == 0 ? c.g_start : c.g_start + (double)i * c.g_delta;
}

// thread e: start a diffeqsolve over the grid (oracle solve() prologue)
__device__ __forceinline__ void ctl_begin(CtlE& c, const Grid& g, float dt0, int lfp_from, int lfp_to, int pos0) {
    c.g_start = g.start;
    c.g_delta = g.delta;
    c.n = g.n;
    const float t0 = (float)grid_at(g, 0);
    c.t1 = (float)grid_at(g, g.n - 1);
    c.tprev = t0;
    c.tnext = fminf(t0 + dt0, c.t1);
    c.h = 0.0f;
    c.dtn = 0.0f;
    c.si = 0;
    c.lfp_from = lfp_from;
    c.lfp_to = lfp_to;
    c.pos0 = pos0;
    c.keep = 0;
    c.nsave = 0;
    c.acc_steps += c.nsteps;  // carry the previous solve's counters
    c.acc_rej += c.rejected;
    c.nsteps = 0;
    c.rejected = 0;
    c.active = g.n >= 2;
}

// MFMA-layout element ownership: lane holds, for each of its TPW column tiles
// t, accumulator rows q = 0..7 (sin rows) and q+8 (cos rows) of local env
// e(q) = (q&3) + 8(q>>2) + 4(lane>>5) at column i = 32(wave*TPW + t) + (lane&31).
// Workspace records are [slot][column tile][half][lane][4] per workgroup: a
// 2 KiB tile holds the 32 columns x 16 envs a wave's tile touches, laid out so
// that each of the two 16-byte vectors a lane loads (q = 0..3: envs 4h..4h+3,
// q = 4..7: envs 8+4h..) sits at lane*16 in its 1 KiB half -- every record
// load/store instruction covers 8 whole 128-byte lines.
__device__ __forceinline__ int mfma_env(int q, int lane) { return (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5); }

enum { SL_Y0 = 0, SL_F0 = 1, SL_Y1 = 8, SL_CA = 9, SL_CB = 10, SL_CC = 11, SL_W = 12, SL_P = 13, NSLOT = 14 };

// One workgroup's solver records, [slot][N][16 envs] f32, addressed through a
// raw buffer descriptor: wave-uniform descriptor and tile offsets (SGPRs), one
// per-lane byte offset (VGPR).  Keeps the record traffic free of 64-bit VALU
// address math and of per-record address registers (which the compiler would
// hoist out of the stage loop and spill).
struct Slot {
    __amdgpu_buffer_rsrc_t rs;
    int N;
    int ct0;   // first column tile of this wave (wave * TPW), wave-uniform
    int voff;  // lane * 16 bytes (half 0); half 1 at +1024
    // FSAL by renaming (post_step): when every active env of the workgroup
    // accepts its step, y0 <- y1 and f0 <- f6 swap the two slot pairs instead
    // of copying records; par = 1 while they are swapped (wave-uniform)
    int par;
#ifdef KURA_DEBUG
    unsigned long long* stats;  // KURA_DEBUG: bounds flag target
#endif
    __device__ int phys(int slot) const {
        const int sw = slot == SL_Y0 ? SL_Y1 : slot == SL_Y1 ? SL_Y0 : slot == SL_F0 ? SL_F0 + 6 : slot == SL_F0 + 6 ? SL_F0 : slot;
        return par ? sw : slot;
    }
    __device__ int soff(int slot, int t) const { return (phys(slot) * N + 32 * (ct0 + t)) * 64; }
    // KURA_DEBUG: the 16 bytes at voff (+1024) + soff lie inside the NSLOT * N * 16 floats of the pair
    __device__ void check(int slot, int t) const {
        KDBG_CHECK(stats, slot >= 0 && slot < NSLOT && ct0 + t >= 0 && (ct0 + t) * 32 < N &&
                              voff + 1024 + soff(slot, t) + 16 <= NSLOT * N * 16 * 4);
    }
};
// the records of workgroup pair `pair`, this wave's tiles from ct0
__device__ __forceinline__ Slot make_slot(DevParamsK& p, int pair, int N, int ct0) {
    const int lane = threadIdx.x & 63;
    Slot s{__builtin_amdgcn_make_buffer_rsrc((void*)uniform_ptr(p.R + (size_t)pair * NSLOT * N * 16), 0,
                                             NSLOT * N * 16 * 4, 0x00020000),
           N, ct0, lane * 16, 0};
#ifdef KURA_DEBUG
    s.stats = uniform_ptr(p.stats);
#endif
    return s;
}

__device__ __forceinline__ void split8(const floatx4& a, const floatx4& b, float (&v)[8]) {
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
// (record loads / stores keep the default cache policy, aux 0: nt, meant to
// keep the record stream from evicting alpha in L2, cost 3.6 % on the loads
// -- a lane's re-reads of its records hit L2 -- and 0.7 % on the stores,
// profiles/r06_record_nt_ab.txt)
// lane's two env groups: half 0 -> envs 4h..4h+3, half 1 -> envs 8+4h..8+4h+3
__device__ __forceinline__ void load8(const Slot& w, int slot, int t, float (&v)[8]) {
    w.check(slot, t);
    const floatx4 a = __builtin_bit_cast(
        floatx4, __builtin_amdgcn_raw_buffer_load_b128(w.rs, w.voff, w.soff(slot, t), 0));
    const floatx4 b = __builtin_bit_cast(
        floatx4, __builtin_amdgcn_raw_buffer_load_b128(w.rs, w.voff + 1024, w.soff(slot, t), 0));
    split8(a, b, v);
}
// Store-data hazard ("The round-2 miscompiles,
// root-caused").  A buffer_store_dwordx4 reads its four data VGPRs after
// issue; on gfx950 a VALU write to one of them within the next 2
// instructions can land first, and the store then writes the NEW value for
// some lanes (observed: dword 1 of the vector, lanes 12-15 of every 16).
// LLVM's hazard recognizer inserts those 2 wait states after global / flat /
// scratch stores, but after a MUBUF store only when its soffset is NOT a
// register (GCNHazardRecognizer::createsVALUHazard).  Record stores therefore
// carry their whole offset in the VGPR and soffset = 0, which puts them under
// the recognizer's guard; the asm makes the lane offset opaque so the
// per-(slot, tile) adds are not hoisted into long-lived registers.
// tools/check_store_hazards.py verifies the shipped machine code (a build
// gate: __graft_entry__.build, tests/test_store_hazards.py); the unguarded
// form is kept only as profiles/r04_sgpr_soffset_store.patch, which the test
// builds to show that the checker flags it.
__device__ __forceinline__ int opaque_vgpr(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ void store_rec_b128(const floatx4& v, __amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, v), rs, opaque_vgpr(voff) + soff, 0, 0);
}
__device__ __forceinline__ void store8(const Slot& w, int slot, int t, const float (&v)[8]) {
    // raw buffer stores through the same wave-uniform descriptor as the
    // loads.  Every record is written and read back only by the lane that owns
    // it, and one wave's vector-memory operations complete in issue order, so
    // no wait is needed between a record store and a later load of it.
    // (Round 1 used global stores here after an unexplained record loss at
    // N=256 during development; it does not reproduce at the commit that
    // introduced the workaround or at any later one)
    w.check(slot, t);
    const floatx4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    store_rec_b128(a, w.rs, w.voff, w.soff(slot, t));
    store_rec_b128(b, w.rs, w.voff + 1024, w.soff(slot, t));
}

// f = fmaf(kn, fmaf(c, P, -(s*Q)), omega) + pulse  ->  slot F0 + stage
// (omega and pulse come from their records, SL_W / SL_P, written at the
// start of the solve; all TPW tiles' loads are issued before the first use)
// (split groups read this part's sin/cos from its published global image)
template <int TPW, bool XL>
__device__ __forceinline__ void coupling_epilogue(DevParamsK& __restrict__ p, const Slot& ws, const float* __restrict__ Xs,
                                                  const float* __restrict__ xown, const floatx16 (&acc)[TPW],
                                                  int stage, bool pulse_on) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float w[TPW][8], u[TPW][8];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        load8(ws, SL_W, t, w[t]);
        if (pulse_on) {
            load8(ws, SL_P, t, u[t]);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) u[t][q] = 0.0f;  // still added: x + 0 is not folded (signed zeros)
        }
    }
    float knq[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) knq[q] = s_kn[mfma_env(q, lane)];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int i = 32 * (wave * TPW + t) + (lane & 31);
        float f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = mfma_env(q, lane);
            const float P = acc[t][q], Q = acc[t][q + 8];
            float sn, cs;
            if constexpr (XL) {
                sn = xown[xs_idx(e, i)];
                cs = xown[xs_idx(16 + e, i)];
            } else {
                sn = Xs[xs_idx(e, i)];
                cs = Xs[xs_idx(16 + e, i)];
            }
            const float tq = sn * Q;
            const float coup = __builtin_fmaf(cs, P, -tq);
            f[q] = __builtin_fmaf(knq[q], coup, w[t][q]) + u[t][q];
        }
        store8(ws, SL_F0 + stage, t, f);
    }
}

// ys = y0 + chain_j(kA[S][j] * (h f_j)), j < S, zero coefficients skipped
// (the oracle's order: fp32 products h*f_j, the first term a product, the
// rest fmas, then y0 + the chain)
template <int S>
__device__ __forceinline__ void stage_ys(const float (&y0)[8], const float (&h)[8], const float (&f)[6][8],
                                         float (&ys)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        if constexpr (S == 0) {
            ys[q] = y0[q];
        } else {
            float acc = kA[S][0] * (h[q] * f[0][q]);
            if constexpr (S > 1 && kA[S][1] != 0.0f) acc = __builtin_fmaf(kA[S][1], h[q] * f[1][q], acc);
            if constexpr (S > 2) acc = __builtin_fmaf(kA[S][2], h[q] * f[2][q], acc);
            if constexpr (S > 3) acc = __builtin_fmaf(kA[S][3], h[q] * f[3][q], acc);
            if constexpr (S > 4) acc = __builtin_fmaf(kA[S][4], h[q] * f[4][q], acc);
            if constexpr (S > 5) acc = __builtin_fmaf(kA[S][5], h[q] * f[5][q], acc);
            ys[q] = y0[q] + acc;
        }
    }
}

// Stage input ys = y0 + chain_j(A[s][j] * h*f_j) (zero coefficients skipped,
// as in the oracle), theta = fmod(ys, 2pi), sin/cos into the LDS operand.
// Stage 0 is the solve's initial RHS at y0.  Tiles are software-pipelined:
// the records of tile t+1 are requested before tile t is computed.  Every
// f_j comes from its record, the newest (f_{s-1}) included: handing it over
// in registers from the epilogue (round 1) only made the compiler spill it
// across the stage barrier -- 32 dwords per lane per sweep to scratch and
// back -- and cost 4 % of the step.
template <int TPW>
__device__ __forceinline__ void stage_input(const Slot& ws, float* Xs, int s STAMP_PARAMS) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float h[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) h[q] = s_ctl[mfma_env(q, lane)].h;
    const int nmem = s;  // f_0 .. f_{s-1}
    float y0[2][8], f[2][6][8];
    auto fetch = [&](int t, int b) __attribute__((always_inline)) {
        load8(ws, SL_Y0, t, y0[b]);
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (j < nmem) load8(ws, SL_F0 + j, t, f[b][j]);
    };
#ifdef KURA_STAMPS_SI
    // diagnostic: no prefetch; per tile: record-load latency (16), arithmetic
    // (17), LDS operand writes (18) -- the compiler moves arithmetic across the
    // (17) boundary, so read 17 + 18 together
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int b = 0;
        STAMP(19);
        fetch(t, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        STAMP(16);
#else
    fetch(0, 0);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int b = t & 1;
        if (t + 1 < TPW) fetch(t + 1, b ^ 1);
#endif
        const int i = 32 * (wave * TPW + t) + (lane & 31);
        float ys[8];
        int slow = 0;
        // one uniform branch per tile to a chain with the stage's tableau row
        // as immediates (a runtime-indexed row was a scalar load plus an
        // lgkmcnt(0) wait per term and element, which also drained the LDS
        // writes of the tile before)
        switch (s) {
            case 0: stage_ys<0>(y0[b], h, f[b], ys); break;
            case 1: stage_ys<1>(y0[b], h, f[b], ys); break;
            case 2: stage_ys<2>(y0[b], h, f[b], ys); break;
            case 3: stage_ys<3>(y0[b], h, f[b], ys); break;
            case 4: stage_ys<4>(y0[b], h, f[b], ys); break;
            case 5: stage_ys<5>(y0[b], h, f[b], ys); break;
            default: stage_ys<6>(y0[b], h, f[b], ys); break;
        }
        // theta = fmod(ys, 2pi_f) folded into the sincos reduction
        // (kdm_sincos_fmod2pi, kura_detmath.h): branch-free for the tile
#ifdef KURA_STAMPS_SI
        float snv[8], csv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int qd;
            const float r = kdm_fold_reduce(ys[q], &qd, &slow);
            kdm_sincos_red(r, qd, &snv[q], &csv[q]);
        }
        asm volatile("" ::: "memory");
        STAMP(17);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = mfma_env(q, lane);
            Xs[xs_idx(e, i)] = snv[q];
            Xs[xs_idx(16 + e, i)] = csv[q];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        STAMP(18);
#else
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float sn, cs;
            int qd;
            const float r = kdm_fold_reduce(ys[q], &qd, &slow);
            kdm_sincos_red(r, qd, &sn, &cs);
            const int e = mfma_env(q, lane);
            Xs[xs_idx(e, i)] = sn;
            Xs[xs_idx(16 + e, i)] = cs;
        }
#endif
        if (__builtin_expect(__any(slow), 0)) {  // some |y| >= 2^22 (never in practice): exact fmod path
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float sn, cs;
                kdm_sincos_fmod2pi(ys[q], &sn, &cs);
                const int e = mfma_env(q, lane);
                Xs[xs_idx(e, i)] = sn;
                Xs[xs_idx(16 + e, i)] = cs;
            }
        }
        if (s == 6) store8(ws, SL_Y1, t, ys);
    }
}

// RM reduction (kura_detmath.h): per-lane partials (t order) -> 32-lane xor
// butterfly -> s_red[k][wave][e]; the caller barriers, then thread e adds the
// 8 wave totals in wave order.
//
// Only lanes 0 and 32 need the butterfly's result, so it is evaluated as the
// same addition tree without shuffling through LDS: xor 16 crosses DPP rows
// (ds_swizzle, bit-mask mode), then DPP row_shl:8/4/2/1 hand lane c+o's
// partial to lane c -- at lane 0 this adds exactly the pairs the xor
// butterfly adds there ((v0+v16) + (v8+v24)) + ..., a bit-exact twin of
// oracle_rm_f32 (other lanes end with values nobody reads).
__device__ __forceinline__ float dpp_shl(float v, int ctrl_sel) {
    int x = __float_as_int(v);
    switch (ctrl_sel) {  // row_shl:N = 0x100 + N (lane i reads lane i+N of its row of 16)
        case 8: x = __builtin_amdgcn_mov_dpp(x, 0x108, 0xF, 0xF, false); break;
        case 4: x = __builtin_amdgcn_mov_dpp(x, 0x104, 0xF, 0xF, false); break;
        case 2: x = __builtin_amdgcn_mov_dpp(x, 0x102, 0xF, 0xF, false); break;
        default: x = __builtin_amdgcn_mov_dpp(x, 0x101, 0xF, 0xF, false); break;
    }
    return __int_as_float(x);
}
__device__ __forceinline__ float rm_half_total(float v) {
    v = v + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));  // xor 16 (and 0x1F)
    v = v + dpp_shl(v, 8);
    v = v + dpp_shl(v, 4);
    v = v + dpp_shl(v, 2);
    v = v + dpp_shl(v, 1);
    return v;
}
__device__ __forceinline__ double dpp_shl_d(double v, int n) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __float_as_uint(dpp_shl(__uint_as_float((uint32_t)u), n));
    const uint32_t hi = __float_as_uint(dpp_shl(__uint_as_float((uint32_t)(u >> 32)), n));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double rm_half_total_d(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)u, 0x401F);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(u >> 32), 0x401F);
    v = v + __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    v = v + dpp_shl_d(v, 8);
    v = v + dpp_shl_d(v, 4);
    v = v + dpp_shl_d(v, 2);
    v = v + dpp_shl_d(v, 1);
    return v;
}
__device__ __forceinline__ void rm_publish(const float (&part)[8], int k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = rm_half_total(part[q]);
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if ((lane & 31) == 0) s_red[k][wave][mfma_env(q, lane)] = v[q];
}
__device__ __forceinline__ void rm_publish_d(const double (&part)[8], int k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = rm_half_total_d(part[q]);
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if ((lane & 31) == 0) s_redd[k][wave][mfma_env(q, lane)] = v[q];
}
__device__ __forceinline__ float rm_total(int e, int k) {
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) tot = tot + s_red[k][w][e];
    return tot;
}
__device__ __forceinline__ double rm_total_d(int e, int k) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) tot = tot + s_redd[k][w][e];
    return tot;
}

// ---- split groups (N > 1024) ---------------------------------------------
// A workgroup's share of one env group.  For N <= 1024 there is one part
// (npart = 1, col0 = 0) and nothing is exchanged.
struct Part {
    int ng;       // oscillators per env (N)
    int col0;     // first oscillator (global column) owned by this workgroup
    int part;     // 0 .. npart-1
    int npart;
    int group;    // envs [16 group, 16 group + 16)
    int pair;     // group * npart + part: index of this workgroup's records
    unsigned ep;  // group exchanges done so far (identical in every part)
    int xs_n;     // sin/cos images published so far (selects the image buffer)
};


typedef __attribute__((address_space(1))) unsigned gu32;

// Payload stores of a group exchange are write-through (sc1), so the
// producer needs no L2 write-back (no release fence): CDNA guide,
// Guideline 16 R1.  The trailing s_nop covers the store-data hazard the
// compiler cannot see through inline asm.
__device__ __forceinline__ void store_sc1_x4(float* dst, const floatx4& v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
}

// Arrive at / wait for the group's barrier number ep+1: every storing wave
// drains its sc1 payload stores, the workgroup barrier, one agent-scope
// atomic arrival, a bounded relaxed poll, one agent-scope acquire (drops this
// CU's L1 lines; L2 is not evicted), the workgroup barrier.  A poll that never
// completes (a part not resident) gives up after ~1 s and raises stats flag
// bit 4 (every later barrier of the launch then gives up at once) instead of
// hanging the GPU.
__device__ __noinline__ void group_barrier(DevParamsK& pin, Part& pt) {
    DevParamsK& p = *uniform_ptr(&pin);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    pt.ep += 1;
    if (threadIdx.x == 0) {
        gu32* cnt = (gu32*)uniform_ptr(p.gcnt + (size_t)pt.group * 16);
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = pt.ep * (unsigned)pt.npart;
        unsigned spins = 0;
        while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(2);
            // after one timeout every later barrier of the launch gives up at once
            if (++spins > XL_SPIN_MAX ||
                (__hip_atomic_load((__attribute__((address_space(1))) unsigned long long*)&p.stats[3],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &
                 (unsigned long long)KURA_F_BARRIER)) {
                atomicOr(&p.stats[3], (unsigned long long)KURA_F_BARRIER);
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}

// Group-wide totals of per-env partial sums: thread e (< 16) passes its
// part's values v[k] (k < nk); on return it holds 0 + part_0 + part_1 + ...
// (part order) -- the RM order extended over parts (oracle_rm_*).
template <int NK>
__device__ __forceinline__ void group_sum(DevParamsK& p, Part& pt, float (&vf)[NK], double (&vd)[NK], int nk,
                                          bool with_d) {
    const int tid = threadIdx.x;
    const int grp = __builtin_amdgcn_readfirstlane(pt.group), npart = __builtin_amdgcn_readfirstlane(pt.npart);
    const int part = __builtin_amdgcn_readfirstlane(pt.part);
    const size_t base = ((size_t)grp * 2 + (__builtin_amdgcn_readfirstlane(pt.ep) & 1)) * npart * (RC * E_WG);
    float* xr = p.xred + base;
    double* xd = p.xredd + base;
    // write-through (sc1) stores of this part's partials by all 64 lanes of
    // wave 0 (a scalar branch): lanes >= E_WG get an offset past the
    // descriptor's range, which the hardware drops -- no exec-masked store
    // (hazards)
    if (__builtin_amdgcn_readfirstlane(tid >> 6) == 0) {
        constexpr int kSc1 = 16;          // cache policy: sc1 (write-through to memory)
        constexpr int kDrop = 0x7ffffff0;
        const bool wd = __builtin_amdgcn_readfirstlane((int)with_d) != 0;
        const __amdgpu_buffer_rsrc_t rf =
            __builtin_amdgcn_make_buffer_rsrc((void*)uniform_ptr(xr), 0, npart * RC * E_WG * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rd =
            __builtin_amdgcn_make_buffer_rsrc((void*)uniform_ptr(xd), 0, npart * RC * E_WG * 8, 0x00020000);
        for (int k = 0; k < nk; ++k) {
            const int o = (part * RC + k) * E_WG + tid;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vf[k]), rf, tid < E_WG ? o * 4 : kDrop, 0, kSc1);
            if (wd) {
                const uint64_t u = (uint64_t)__double_as_longlong(vd[k]);
                typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{(unsigned)u, (unsigned)(u >> 32)}, rd,
                                                      tid < E_WG ? o * 8 : kDrop, 0, kSc1);
            }
        }
    }
    group_barrier(p, pt);
    if (tid < E_WG)
        for (int k = 0; k < nk; ++k) {
            float a = 0.0f;
            double b = 0.0;
            for (int q = 0; q < npart; ++q) {
                a = a + xr[(q * RC + k) * E_WG + tid];
                if (with_d) b = b + xd[(q * RC + k) * E_WG + tid];
            }
            vf[k] = a;
            vd[k] = b;
        }
}

// Publish this part's sin/cos image (LDS, xl_img(TPW) floats) into the group's
// image buffer and wait until every part has published its own.
template <int TPW>
__device__ __forceinline__ const float* group_publish_x(DevParamsK& p, Part& pt, const float* Xs) {
    constexpr int XL_IMG = xl_img(TPW);
    const int grp = __builtin_amdgcn_readfirstlane(pt.group), npart = __builtin_amdgcn_readfirstlane(pt.npart);
    const size_t img = ((size_t)grp * 2 + (__builtin_amdgcn_readfirstlane(pt.xs_n) & 1)) * npart * XL_IMG;
    float* dst = uniform_ptr(p.xg + img + (size_t)__builtin_amdgcn_readfirstlane(pt.part) * XL_IMG);
    const floatx4* src = (const floatx4*)Xs;
    for (int k = threadIdx.x; k < XL_IMG / 4; k += NTHREADS) store_sc1_x4(dst + 4 * k, src[k]);
    group_barrier(p, pt);
    pt.xs_n += 1;
    return p.xg + img;
}

// The error estimate and dense-output coefficients of one tile of the step
// just taken (diffrax Dopri5: Shampine error weights kE, 4th-order
// interpolation c_mid weights kM; oracle solve()): part[q] += (err/scale)^2,
// CA/CB/CC records stored.  k_j = h f_j.
template <typename DP>
__device__ __forceinline__ void err_dense_tile(const DP& p, const Slot& ws, int t, const float (&h)[8],
                                               const float (&y0)[8], const float (&y1)[8], const float (&f0)[8],
                                               const float (&f2)[8], const float (&f3)[8], const float (&f4)[8],
                                               const float (&f5)[8], const float (&f6)[8], float (&part)[8]) {
    float ca[8], cb[8], cc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float k0 = h[q] * f0[q], k2 = h[q] * f2[q], k3 = h[q] * f3[q], k4 = h[q] * f4[q],
                    k5 = h[q] * f5[q], k6 = h[q] * f6[q];
        float er = kE[0] * k0;
        er = __builtin_fmaf(kE[2], k2, er);
        er = __builtin_fmaf(kE[3], k3, er);
        er = __builtin_fmaf(kE[4], k4, er);
        er = __builtin_fmaf(kE[5], k5, er);
        er = __builtin_fmaf(kE[6], k6, er);
        const float a0 = fabsf(y0[q]), a1 = fabsf(y1[q]);
        const float mx = a0 > a1 ? a0 : a1;
        const float den = p.atol + mx * p.rtol;
        const float qe = er / den;
        part[q] = part[q] + qe * qe;
        float acc = kM[0] * k0;
        acc = __builtin_fmaf(kM[2], k2, acc);
        acc = __builtin_fmaf(kM[3], k3, acc);
        acc = __builtin_fmaf(kM[4], k4, acc);
        acc = __builtin_fmaf(kM[5], k5, acc);
        acc = __builtin_fmaf(kM[6], k6, acc);
        const float yy0 = y0[q], yy1 = y1[q];
        const float ym = yy0 + acc;
        ca[q] = ((2.0f * (k6 - k0)) - (8.0f * (yy1 + yy0))) + (16.0f * ym);
        cb[q] = ((((5.0f * k0) - (3.0f * k6)) + (18.0f * yy0)) + (14.0f * yy1)) - (32.0f * ym);
        cc[q] = (((k6 - (4.0f * k0)) - (11.0f * yy0)) - (5.0f * yy1)) + (16.0f * ym);
    }
    store8(ws, SL_CA, t, ca);
    store8(ws, SL_CB, t, cb);
    store8(ws, SL_CC, t, cc);
}

// After the 7th stage: error norm, accept/reject, dense-output saves with
// LFP, FSAL -- for all 16 envs, every wave on its own columns.
// One pass of post_step's saves: rounds r0 .. r0+nk-1 (nk = min(RCX, nrounds - r0))
// evaluated from the dense-output records of every tile, LFP partials reduced
// in RM order, samples stored by thread e.  RCX is a compile-time bound on the
// rounds of a pass (register arrays); rounds past nk are skipped.
// Rounds r0 == 0 (the first pass) take their abscissae from post_step's
// decision section (save_rounds_setup), later passes form them here.
template <int RCX>
__device__ __forceinline__ void save_rounds_setup(const CtlE& c, int e, int r0) {
    for (int k = 0; k < RCX; ++k) {
        const int r = r0 + k;
        int fl = 0;
        float th = 0.0f;
        if (r < c.nsave) {
            const int si = c.sv_si + r;
            const float ts = (float)grid_at_c(c, si);
            th = (ts - c.sv_tprev) / (c.sv_tnext - c.sv_tprev);
            fl = 1 | ((si >= c.lfp_from && si < c.lfp_to) ? 2 : 0) | ((si == c.n - 1) ? 4 : 0);
        }
        s_theta[e][k] = th;
        s_rflag[e][k] = fl;
    }
}

template <int TPW, bool XL, int RCX, bool RS>
__device__ __forceinline__ void save_pass(DevParamsK& __restrict__ p, const Slot& ws, int env_base, Part& pt,
                                          const float (&h)[8], int r0, int nrounds, bool gauss STAMP_PARAMS) {
    constexpr bool to_ring = RS;   // a reset's transient (ring, rows_tr) or a step's solve (samples, rows)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int NG = XL ? __builtin_amdgcn_readfirstlane(pt.ng) : TPW * 256;
    const int col0 = XL ? __builtin_amdgcn_readfirstlane(pt.col0) : 0;
    const int nk = nrounds - r0 < RCX ? nrounds - r0 : RCX;
    const int Bn = p.B;
    // per-round flag bits, 3 per round: LFP rows, and LFP or final rows
    constexpr int kLfp = (int)(02222222222u & ((1u << (3 * RCX)) - 1u));
    constexpr int kEval = (int)(06666666666u & ((1u << (3 * RCX)) - 1u));
    // (1) abscissa and flags of every (env, round) of the pass: one thread
    // each (the first pass's were formed in post_step's decision section)
    if (r0 > 0) {
        if (tid < E_WG * RCX) {
            const int e = tid % E_WG, k = tid / E_WG;
            const CtlE& c = s_ctl[e];
            const int r = r0 + k;
            int fl = 0;
            float th = 0.0f;
            if (r < c.nsave) {
                const int si = c.sv_si + r;
                const float ts = (float)grid_at_c(c, si);
                th = (ts - c.sv_tprev) / (c.sv_tnext - c.sv_tprev);
                fl = 1 | ((si >= c.lfp_from && si < c.lfp_to) ? 2 : 0) | ((si == c.n - 1) ? 4 : 0);
            }
            s_theta[e][k] = th;
            s_rflag[e][k] = fl;
        }
        lds_barrier();
    }
    STAMP(11);
    float th[RCX][8];
    int fl[8];
    int anyl = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = mfma_env(q, lane);
        int f = 0;
#pragma unroll
        for (int k = 0; k < RCX; ++k) {
            th[k][q] = s_theta[e][k];
            f |= s_rflag[e][k] << (3 * k);
        }
        fl[q] = f;
        anyl |= f & kLfp;
    }
    float pn[RCX][8];
    double pg[RCX][8];
#pragma unroll
    for (int k = 0; k < RCX; ++k)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            pn[k][q] = 0.0f;
            pg[k][q] = 0.0;
        }
    // identical in every wave: each wave holds all 16 envs
    const int anyw = __any(anyl) ? (anyl | __shfl_xor(anyl, 32, 64)) : 0;
    // rows that feed neither an LFP sample nor the final state (the first
    // 3999 - W saves of the reset transient) need no evaluation at all --
    // unless the step's rows are captured (kura_set_row_capture)
    const int flor = fl[0] | fl[1] | fl[2] | fl[3] | fl[4] | fl[5] | fl[6] | fl[7];
    constexpr int kSave = (int)(01111111111u & ((1u << (3 * RCX)) - 1u));
    // captured rows: a step's into rows ([B][KURA_S_MAX+1][N], row = LFP
    // position), a reset's into rows_tr ([B][n_tr][N], row = save index)
    constexpr bool reset_rows = RS;
    // (p is read through vector loads in the called solver: the capture switch
    // and the descriptor fields are made wave-uniform, else the capture branch
    // is divergent and its stores become exec-masked waterfall loops)
    const bool capture = __builtin_amdgcn_readfirstlane((int)(reset_rows ? p.rows_tr != nullptr : p.rows != nullptr)) != 0;
    const int crow = __builtin_amdgcn_readfirstlane(reset_rows ? p.n_tr : KURA_S_MAX + 1);   // captured rows per env
    const bool eval_rows = __any(flor & (capture ? kSave : kEval));  // rows to evaluate in any round
    int fin = 0;  // wave-uniform: rounds holding some env's final row (bit k)
#pragma unroll
    for (int k = 0; k < RCX; ++k) fin |= __any((flor >> (3 * k)) & 4) ? (1 << k) : 0;
    // final state and captured rows: raw buffer stores through descriptors
    // over this env group's valid envs, one unconditional store per element;
    // an element that is not stored gets an offset past the range, which the
    // hardware drops.  (Per-element exec-masked flat stores here lost almost
    // every final-state store of the split kernel with parts of 512 in some
    // builds -- the sums of the same pass were right -- DESIGN.md section 5.)
    // (env_base reaches this called solver in a VGPR: made wave-uniform, else
    // the descriptors below are divergent and every store through them becomes
    // a waterfall loop under an exec mask)
    const int nvalid = __builtin_amdgcn_readfirstlane(Bn - env_base < E_WG ? Bn - env_base : E_WG);
    const __amdgpu_buffer_rsrc_t ys = __builtin_amdgcn_make_buffer_rsrc(
        (void*)uniform_ptr(p.y + (size_t)env_base * NG), 0, nvalid * NG * 4, 0x00020000);
    float* const rows = reset_rows ? p.rows_tr : p.rows;
    const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(
        (void*)uniform_ptr(capture ? rows + (size_t)env_base * crow * NG : p.y), 0,
        __builtin_amdgcn_readfirstlane(capture ? nvalid * crow * NG * 4 : 0), 0x00020000);
    constexpr int kDrop = 0x7ffffff0;   // past every range: the store is dropped
    int rbase[8];  // captured row index of round 0 of this pass: sol_state_ row si - lfp_from + pos0 (step), si (reset)
    if (capture) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const CtlE& c = s_ctl[mfma_env(q, lane)];
            rbase[q] = reset_rows ? c.sv_si + r0 : c.sv_si + r0 - c.lfp_from + c.pos0;
        }
    }
    // (2) dense output + LFP partials: every (round, env) of a tile is
    // evaluated without branching (rows that are not saved or feed no LFP
    // sample are computed and discarded by a select: the partial sums see
    // exactly the additions of the branchy form, in the same order)
    // Split groups: tiles are visited one 16-byte record half at a time (envs q = 4h..4h+3),
    // all TPW tiles of half 0, then of half 1, with the five records of the
    // next (tile, half) in flight while the current one is evaluated.  Every
    // (round, env) partial still adds its tiles in t order, so the sums are
    // those of a tile-by-tile pass (bit-exact); a prefetched half costs the
    // registers one whole tile used to.
    // (K1 / K2 keep the tile-by-tile pass: same-box A/B, the half-tile form
    // cost the N=1024 step 0.5 % and gained its reset 0.4 %,
    // profiles/r03_savepass_ab.txt; the split strong form gained 1.5 %)
    if (XL && eval_rows) {
        float rc[5][4];  // CA, CB, CC, F0, Y0 of the current (tile, half)
        auto load_half = [&](int t, int hh, float (&r)[5][4]) __attribute__((always_inline)) {
            const int sl[5] = {SL_CA, SL_CB, SL_CC, SL_F0, SL_Y0};
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                ws.check(sl[j], t);
                const floatx4 v = __builtin_bit_cast(
                    floatx4, __builtin_amdgcn_raw_buffer_load_b128(ws.rs, ws.voff, ws.soff(sl[j], t) + hh * 1024, 0));
                r[j][0] = v[0]; r[j][1] = v[1]; r[j][2] = v[2]; r[j][3] = v[3];
            }
        };
        load_half(0, 0, rc);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
#pragma unroll 1
            for (int t = 0; t < TPW; ++t) {
                const int i = 32 * (wave * TPW + t) + (lane & 31);
                const bool last = t + 1 == TPW;
                float rn[5][4];
                if (!(hh == 1 && last)) load_half(last ? 0 : t + 1, last ? 1 : hh, rn);
                double G[4];
                if (gauss) {
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        int env = env_base + mfma_env(4 * hh + qq, lane);
                        env = env < Bn ? env : Bn - 1;
                        G[qq] = p.g_rec[(size_t)env * NG + col0 + i];
                    }
                }
#ifdef KURA_STAMPS
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // attribute the record-load wait (diagnostic build)
                STAMP(12);
#endif
                float k0[4];
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) k0[qq] = h[4 * hh + qq] * rc[3][qq];
#pragma unroll
                for (int k = 0; k < RCX; ++k) {
                    if (k >= nk) break;  // wave-uniform: past every env's last save of this step
                    float v[4];
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int q = 4 * hh + qq;
                        const int f = fl[q] >> (3 * k);
                        const float x = th[k][q];
                        float w = rc[0][qq] * x + rc[1][qq];
                        w = w * x + rc[2][qq];
                        w = w * x + k0[qq];
                        w = w * x + rc[4][qq];
                        v[qq] = w;
                        const float cr = kdm_cosf(w);
                        pn[k][q] = (f & 2) ? pn[k][q] + cr : pn[k][q];
                        if (gauss) pg[k][q] = (f & 2) ? pg[k][q] + (double)cr * G[qq] : pg[k][q];
                    }
                    if ((fin >> k) & 1) {  // the solve's last row: the new state
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) {
                            const int q = 4 * hh + qq;
                            const int off = (mfma_env(q, lane) * NG + col0 + i) * 4;
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[qq]), ys,
                                                                  ((fl[q] >> (3 * k)) & 4) ? off : kDrop, 0, 0);
                        }
                    }
                    if (capture) {
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) {
                            const int q = 4 * hh + qq;
                            const int off = ((mfma_env(q, lane) * crow + rbase[q] + k) * NG + col0 + i) * 4;
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[qq]), rws,
                                                                  ((fl[q] >> (3 * k)) & 1) ? off : kDrop, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 5; ++j)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) rc[j][qq] = rn[j][qq];
                STAMP(13);
            }
        }
    }
    // K1 / K2: tile by tile, one round at a time (rounds evaluated as packed
    // FP32 pairs doubled the solver's scratch: step -6 to -11 %, reset +51 %,
    // profiles/r06_save_packed_ab.txt)
#pragma unroll 1
    for (int t = 0; t < (!XL && eval_rows ? TPW : 0); ++t) {
        const int i = 32 * (wave * TPW + t) + (lane & 31);
        float ca[8], cb[8], cc[8], f0[8], y0[8];
        double G[8];
        load8(ws, SL_CA, t, ca);
        load8(ws, SL_CB, t, cb);
        load8(ws, SL_CC, t, cc);
        load8(ws, SL_F0, t, f0);
        load8(ws, SL_Y0, t, y0);
        if (gauss) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                int env = env_base + mfma_env(q, lane);
                env = env < Bn ? env : Bn - 1;
                G[q] = p.g_rec[(size_t)env * NG + col0 + i];
            }
        }
#ifdef KURA_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // attribute the record-load wait (diagnostic build)
        STAMP(12);
#endif
        float k0[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) k0[q] = h[q] * f0[q];
#pragma unroll
        for (int k = 0; k < RCX; ++k) {
            if (k >= nk) break;  // wave-uniform: past every env's last save of this step
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int f = fl[q] >> (3 * k);
                // recorder LFP: an empty slot (no sample, not the state, not
                // captured) skips its dense output, cos and f64 partial --
                // the reset's lockstep passes have many (-20 % on the env1
                // reset); for the naive LFP the branch costs more than it
                // saves (profiles/r05_save_skip_ab.txt)
                v[q] = 0.0f;
                if (gauss && !(f & (capture ? 7 : 6))) continue;
                const float x = th[k][q];
                float w = ca[q] * x + cb[q];
                w = w * x + cc[q];
                w = w * x + k0[q];
                w = w * x + y0[q];
                v[q] = w;
                const float cr = kdm_cosf(w);
                pn[k][q] = (f & 2) ? pn[k][q] + cr : pn[k][q];
                if (gauss) pg[k][q] = (f & 2) ? pg[k][q] + (double)cr * G[q] : pg[k][q];
            }
            if ((fin >> k) & 1) {  // the solve's last row: the new state
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int off = (mfma_env(q, lane) * NG + col0 + i) * 4;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), ys,
                                                          ((fl[q] >> (3 * k)) & 4) ? off : kDrop, 0, 0);
                }
            }
            if (capture) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int off = ((mfma_env(q, lane) * crow + rbase[q] + k) * NG + col0 + i) * 4;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rws,
                                                          ((fl[q] >> (3 * k)) & 1) ? off : kDrop, 0, 0);
                }
            }
        }
        STAMP(13);
    }
#pragma unroll
    for (int k = 0; k < RCX; ++k) {
        if (__any((anyl >> (3 * k)) & 2)) {
            rm_publish(pn[k], k);
            if (gauss) rm_publish_d(pg[k], k);
        }
    }
    (void)anyw;
    lds_barrier();
    STAMP(14);
    // (3) per (env, round) totals in wave order, LFP samples out
    if constexpr (!XL) {
        if (tid < E_WG * RCX) {
            const int e = tid % E_WG, k = tid / E_WG;
            if (s_rflag[e][k] & 2) {
                const CtlE& c = s_ctl[e];
                const float ln = rm_total(e, k) / (float)NG;
                const double lr = gauss ? 0.0 + rm_total_d(e, k) / (double)NG : (double)ln;
                const int pos = c.sv_si + r0 + k - c.lfp_from + c.pos0;
                KDBG_CHECK(p.stats, pos >= 0 && (to_ring ? pos < (p.lfp_tr ? c.n - 1 : p.W) : pos < KURA_S_MAX + 2) &&
                                        env_base + e < p.B);
                if (to_ring) {
                    // (reset: with the transient record on, every row feeds a sample and the ring takes the last W)
                    int rp = pos;
                    if (p.lfp_tr) {
                        p.lfp_tr[(size_t)(env_base + e) * (c.n - 1) + pos] = lr;
                        rp = pos - (c.n - 1 - p.W);
                    }
                    if (rp >= 0) p.ring[(size_t)(env_base + e) * p.W + rp] = lr;
                } else {
                    s_smp_n[e][pos] = ln;
                    s_smp_r[e][pos] = lr;
                }
            }
        }
    } else {
        float ltot[RCX];
        double ltot_d[RCX];
#pragma unroll
        for (int k = 0; k < RCX; ++k) {
            ltot[k] = 0.0f;
            ltot_d[k] = 0.0;
            if (tid < E_WG && (s_rflag[tid][k] & 2)) {
                ltot[k] = rm_total(tid, k);
                if (gauss) ltot_d[k] = rm_total_d(tid, k);
            }
        }
        if (__builtin_amdgcn_readfirstlane(anyw) & kLfp) group_sum<RCX>(p, pt, ltot, ltot_d, RCX, gauss);
        if (tid < E_WG) {
            const CtlE& c = s_ctl[tid];
            for (int k = 0; k < RCX; ++k) {
                if (!(s_rflag[tid][k] & 2)) continue;
                const int si = c.sv_si + r0 + k;
                const float ln = ltot[k] / (float)NG;
                const double lr = gauss ? 0.0 + ltot_d[k] / (double)NG : (double)ln;
                const int pos = si - c.lfp_from + c.pos0;
                KDBG_CHECK(p.stats, pos >= 0 && (to_ring ? pos < (p.lfp_tr ? c.n - 1 : p.W) : pos < KURA_S_MAX + 2) &&
                                        env_base + tid < p.B);
                if (to_ring && pt.part == 0) {
                    int rp = pos;
                    if (p.lfp_tr) {
                        p.lfp_tr[(size_t)(env_base + tid) * (c.n - 1) + pos] = lr;
                        rp = pos - (c.n - 1 - p.W);
                    }
                    if (rp >= 0) p.ring[(size_t)(env_base + tid) * p.W + rp] = lr;
                } else if (!to_ring) {
                    s_smp_n[tid][pos] = ln;
                    s_smp_r[tid][pos] = lr;
                }
            }
        }
    }
    // the next pass rewrites s_theta / s_rflag / s_red; after the last pass
    // nothing reads them before post_step's next barriers
    if (XL || r0 + RCX < nrounds) lds_barrier();
    STAMP(15);
}

// Returns whether any env of the workgroup goes on integrating (uniform).
template <int TPW, bool XL, bool RS>
__device__ __forceinline__ int post_step(DevParamsK& __restrict__ p, Slot& ws, int env_base, Part& pt
                                         STAMP_PARAMS) {
    const int lane = threadIdx.x & 63, tid = threadIdx.x;
    const int NG = XL ? __builtin_amdgcn_readfirstlane(pt.ng) : TPW * 256;   // oscillators per env
    float h[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) h[q] = s_ctl[mfma_env(q, lane)].h;
    // (1) scaled error partials and dense-output coefficients: a pass of its
    // own.  (Folded into the stage-6 epilogue it saves one record round trip
    // and one barrier per Dopri step, yet was 2 % slower in the same-box A/B:
    // the fused epilogue holds the accumulators and the seven records of a
    // tile at once)
    float part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // (kept rolled: the unrolled loop measured 0.4 % slower, same box,
    // profiles/r04_solver_ab.txt)
#pragma unroll 1
    for (int t = 0; t < TPW; ++t) {
        float y0[8], y1[8], f0[8], f2[8], f3[8], f4[8], f5[8], f6[8];
        load8(ws, SL_Y0, t, y0);
        load8(ws, SL_Y1, t, y1);
        load8(ws, SL_F0 + 0, t, f0);
        load8(ws, SL_F0 + 2, t, f2);
        load8(ws, SL_F0 + 3, t, f3);
        load8(ws, SL_F0 + 4, t, f4);
        load8(ws, SL_F0 + 5, t, f5);
        load8(ws, SL_F0 + 6, t, f6);
        err_dense_tile(p, ws, t, h, y0, y1, f0, f2, f3, f4, f5, f6, part);
    }
    rm_publish(part, 0);
    STAMP(5);
    lds_barrier();
    float etot[1] = {tid < E_WG ? rm_total(tid, 0) : 0.0f};
    if constexpr (XL) {
        double dummy[1] = {0.0};
        group_sum<1>(p, pt, etot, dummy, 1, false);
    }
    // (2) thread e: accept/reject, step-size update (diffrax PIDController),
    // then at once the time advance (adapt_step_size + _clip_to_end) and the
    // next step size; the saves below read the step's save index and
    // interval from the sv_* snapshot, and the first save pass's abscissae
    // are formed here too (one section and barrier instead of four)
    const bool gauss = p.rec_kernel == KURA_REC_GAUSSIAN;
    if (tid < E_WG) {
        CtlE& c = s_ctl[tid];
        c.nsave = 0;
        c.keep = 0;
        c.sv_si = c.si;
        c.sv_tprev = c.tprev;
        c.sv_tnext = c.tnext;
        const float mean = etot[0] / (float)NG;
        if (c.active && !(mean <= 3.40282346638528859812e+38f)) {
            // non-finite state or RHS (NaN/Inf reaches the error norm): the
            // solve fails here, as in the oracle (KURA_F_NONFINITE)
            c.flags |= KURA_F_NONFINITE;
            c.active = 0;
        }
        if (c.active) {
            const float err = sqrtf(mean);
            const bool keep = err < 1.0f;
            float fac = 0.9f * kdm_inv_fifth_root(err);
            const float fmn = keep ? 1.0f : 0.2f;
            fac = fac > fmn ? fac : fmn;
            fac = fac < 10.0f ? fac : 10.0f;
            c.dtn = c.h * fac;
            c.keep = keep;
            if (keep) {
                int k = 0;
                while (c.si + k < c.n && (float)grid_at_c(c, c.si + k) <= c.tnext) ++k;
                c.nsave = k;
            }
        }
        if (c.active) {  // time advance (formerly after the saves)
            c.si += c.nsave;
            if (c.keep) c.tprev = c.tnext;
            else c.rejected++;
            float tn = c.tprev + c.dtn;
            c.tprev = fminf(c.tprev, c.t1);
            if (tn > c.t1 - 1e-6f) tn = c.keep ? c.t1 : c.tprev + 0.5f * (c.t1 - c.tprev);
            c.tnext = tn;
            c.nsteps++;
            if (!(c.tprev < c.t1)) c.active = 0;
            if (c.active && c.nsteps >= p.max_steps) {
                c.flags |= KURA_F_MAX_STEPS;
                c.active = 0;
            }
            if (c.active) c.h = c.tnext - c.tprev;   // the next attempt's step
        }
        if (XL || gauss) save_rounds_setup<RC>(c, tid, 0);
        else save_rounds_setup<RC_N>(c, tid, 0);
    }
    lds_barrier();
    // every wave: most save rounds of any env; FSAL mode: 0 no env that goes
    // on integrating accepts (nothing to move), 2 every such env accepts
    // (rename the slot pairs), 1 mixed (select-copy) -- envs that end their
    // solve with this step never read their records again; and whether any
    // env goes on (the solve loop's exit).  Wave-uniform reads of s_ctl.
    int nrounds = 0, allk = 1, anyk = 0, any = 0;
#pragma unroll
    for (int e = 0; e < E_WG; ++e) {
        const CtlE& c = s_ctl[e];
        const int ns = __builtin_amdgcn_readfirstlane(c.nsave);
        const int ac = __builtin_amdgcn_readfirstlane(c.active), kp = __builtin_amdgcn_readfirstlane(c.keep);
        nrounds = ns > nrounds ? ns : nrounds;
        if (ac) {
            allk &= kp;
            anyk |= kp;
            any = 1;
        }
    }
    STAMP(7);
    // (3) saves: up to RCX rounds (save indices) per pass over the records,
    // all envs in parallel; one RM reduction per round and LFP kind
    if (XL || gauss) {
#pragma unroll 1
        for (int r0 = 0; r0 < nrounds; r0 += RC)
            save_pass<TPW, XL, RC, RS>(p, ws, env_base, pt, h, r0, nrounds, gauss STAMP_ARGS);
    } else {
#pragma unroll 1
        for (int r0 = 0; r0 < nrounds; r0 += RC_N)
            save_pass<TPW, XL, RC_N, RS>(p, ws, env_base, pt, h, r0, nrounds, false STAMP_ARGS);
    }
    STAMP(8);
    // (4) accepted envs: y0 <- y1, f0 <- f6 (FSAL).  Envs that are not
    // active any more never read their records again (their final state is
    // out), so when every active env accepts the slot pairs are renamed.
    int kp[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) kp[q] = s_ctl[mfma_env(q, lane)].keep;
    const int fmode = anyk ? (allk ? 2 : 1) : 0;
    if (fmode == 2) ws.par ^= 1;
#pragma unroll 1
    for (int t = 0; t < (fmode == 1 ? TPW : 0); ++t) {
        float y0[8], y1[8], f0[8], f6[8];
        load8(ws, SL_Y0, t, y0);
        load8(ws, SL_Y1, t, y1);
        load8(ws, SL_F0, t, f0);
        load8(ws, SL_F0 + 6, t, f6);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            y0[q] = kp[q] ? y1[q] : y0[q];
            f0[q] = kp[q] ? f6[q] : f0[q];
        }
        store8(ws, SL_Y0, t, y0);
        store8(ws, SL_F0, t, f0);
    }
    STAMP(9);
    // no barrier here: nothing the saves / FSAL wrote (records: per lane; ring,
    // LFP samples: thread e) is read by another thread before the next
    // stage's barrier, and the next stage input only writes the operand,
    // whose last readers (the stage-6 GEMM and epilogue) are behind a barrier
    return any;
}

// One diffeqsolve for the workgroup's 16 envs.  s_ctl must be initialised
// (ctl_begin) and visible before the call.
// The solver is a called function (one call site per kernel; its frame saves
// the callee-saved registers once per solve).  Inlined the kernel needs less
// scratch (648 vs ~1200 B per lane for <4, false>) but the register
// allocation of the combined body spills inside the sweep loop: same-box A/B,
// 0.750 vs 0.788 of the FP32 MFMA peak.
template <int TPW, bool XL, bool SP, bool RS>
__device__ __noinline__ void solve_wg(DevParamsK& __restrict__ pin, float* Xs, int env_base, bool pulse_on,
                                      long long* rhs_count, Part& pt) {
    // (the kernarg segment through the VGPR-passed pointer: vector loads.
    // Made wave-uniform -- scalar loads, which share lgkmcnt with the LDS
    // traffic -- the step was 1.5 % slower in the same-box A/B,
    // profiles/r04_solver_ab.txt)
    DevParamsK& __restrict__ p = pin;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    constexpr int N = TPW * 256;            // oscillators owned by this workgroup
    const int NG = XL ? __builtin_amdgcn_readfirstlane(pt.ng) : N;      // oscillators per env
    const int col0 = XL ? __builtin_amdgcn_readfirstlane(pt.col0) : 0;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pair = __builtin_amdgcn_readfirstlane(pt.pair);
    Slot ws = make_slot(p, pair, N, wv * TPW);
    // records y0 <- state y, omega, pulse (0 while stimulation is OFF, env.py:434)
#pragma unroll 1
    for (int t = 0; t < TPW; ++t) {
        const int i = 32 * (wave * TPW + t) + (lane & 31);
        float v[8], w[8], u[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int env = env_base + mfma_env(q, lane);
            const bool ok = env < p.B;
            env = ok ? env : p.B - 1;  // padded slots: any valid address
            const size_t o = (size_t)env * NG + col0 + i;
            v[q] = ok ? p.y[o] : 0.0f;
            w[q] = p.omega[o];
            u[q] = pulse_on ? p.pulse[o] : 0.0f;
        }
        store8(ws, SL_Y0, t, v);
        store8(ws, SL_W, t, w);
        if (pulse_on) store8(ws, SL_P, t, u);
    }
    asm volatile("" ::: "memory");  // record stores before the first record loads
    if (tid < E_WG) {  // visible to the epilogue after the first stage barrier
        const int env = env_base + tid;
        s_kn[tid] = p.kn_env[env < p.B ? env : p.B - 1];
    }
    STAMP_DECL
    long long nrhs = 0;
    int s = 0;  // stage 0 = initial RHS at y0 (FSAL seed)
    stage_input<TPW>(ws, Xs, 0 STAMP_ARGS);
    STAMP(0);
    for (;;) {
        floatx16 acc[TPW];
        lds_barrier();
        STAMP(1);
        const float* xown = nullptr;
        if constexpr (XL) {
            const float* xgrp = uniform_ptr(group_publish_x<TPW>(p, pt, Xs));   // all parts' images of this stage
            xown = xgrp + (size_t)__builtin_amdgcn_readfirstlane(pt.part) * xl_img(TPW);
            STAMP(16);  // split groups: image publish + group barrier (slot 16 is free outside KURA_STAMPS_SI)
            if constexpr (SP) {
#ifdef KURA_DEBUG
                unsigned long long* dbg = uniform_ptr(p.stats);
#else
                unsigned long long* dbg = nullptr;
#endif
                if constexpr (TPW > KURA_XL_SP_STAGED_MAXTPW)
                    coupling_gemm_xl_bf16x3_kb<TPW>(xgrp, p.alpha_sw, Xs, NG, col0, acc, dbg STAMP_ARGS);
                else
                    coupling_gemm_xl_bf16x3<TPW>(xgrp, p.alpha_sw, Xs, NG, col0, acc, dbg STAMP_ARGS);
            } else
                coupling_gemm_xl<TPW>(xgrp, p.alpha_sw, Xs, NG, col0, acc STAMP_ARGS);
        } else {
#ifdef KURA_DEBUG
            coupling_gemm<TPW, SP>(Xs, p.alpha_sw, p.alpha_reuse, acc, uniform_ptr(p.stats));
            if (p.gemm_dump && blockIdx.x == 0 && nrhs < p.gemm_dump_n) {   // the sweep's operand and sums
                float* d = p.gemm_dump + (size_t)nrhs * 2 * 32 * N;
                for (int idx = tid; idx < 32 * N; idx += NTHREADS) d[idx] = Xs[xs_idx(idx / N, idx % N)];
#pragma unroll
                for (int t = 0; t < TPW; ++t)
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        d[32 * N + (size_t)((q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)) * N + 32 * (wave * TPW + t) +
                          (lane & 31)] = acc[t][q];
            }
#else
            if constexpr (SP && RS)   // the reset reads the deduplicated image
                coupling_gemm_bf16x3_dd<TPW>(Xs, p.alpha_dd, p.alpha_dd_bytes, acc);
            else
                coupling_gemm<TPW, SP>(Xs, p.alpha_sw, p.alpha_reuse, acc);
#endif
        }
        STAMP(2);
        coupling_epilogue<TPW, XL>(p, ws, Xs, xown, acc, s, pulse_on);
        STAMP(3);
        lds_barrier();  // every wave is done reading the operand before it is rewritten
        STAMP(4);
        ++nrhs;
        if (s > 0 && s < 6) {
            ++s;
            stage_input<TPW>(ws, Xs, s STAMP_ARGS);
            STAMP(0);
            continue;
        }
        int any;
        if (s == 6) {
            any = post_step<TPW, XL, RS>(p, ws, env_base, pt STAMP_ARGS);   // advances time, sets h
            STAMP(10);
        } else {  // the solve's initial sweep: the first attempt's step size
            if (tid < E_WG && s_ctl[tid].active) s_ctl[tid].h = s_ctl[tid].tnext - s_ctl[tid].tprev;
            any = 0;
#pragma unroll
            for (int e = 0; e < E_WG; ++e) any |= __builtin_amdgcn_readfirstlane(s_ctl[e].active);
            lds_barrier();
            STAMP(6);
        }
        if (any == 0) break;
        // stage 1 of the next Dopri step (f_0: the stage-0 record, or the
        // FSAL select of post_step)
        s = 1;
        stage_input<TPW>(ws, Xs, 1 STAMP_ARGS);
        STAMP(0);
    }
    STAMP_FLUSH(p);
    *rhs_count += nrhs;
}

__device__ __forceinline__ void flush_stats(DevParamsK& p, long long rhs, int env_base) {
    if (threadIdx.x != 0) return;
    unsigned long long steps = 0, rej = 0, flags = 0;
    for (int e = 0; e < E_WG; ++e) {
        if (env_base + e >= p.B) continue;
        steps += s_ctl[e].acc_steps + s_ctl[e].nsteps;
        rej += s_ctl[e].acc_rej + s_ctl[e].rejected;
        flags |= s_ctl[e].flags;
    }
    atomicMax(&p.stats[0], (unsigned long long)rhs);
    atomicAdd(&p.stats[1], steps);
    atomicAdd(&p.stats[2], rej);
    if (flags) atomicOr(&p.stats[3], flags);
    atomicAdd(&p.stats[4], (unsigned long long)rhs);
    atomicAdd(&p.stats[5], steps);
    atomicAdd(&p.stats[6], (unsigned long long)rhs);
    atomicAdd(&p.stats[7], rej);
}

// Kernel prologue: zero every env's control slot.
__device__ __forceinline__ void ctl_clear() {
    if (threadIdx.x < E_WG) {
        CtlE& c = s_ctl[threadIdx.x];
        c.active = 0;
        c.nsteps = c.rejected = c.flags = 0;
        c.acc_steps = c.acc_rej = 0;
        c.n = 0;
        c.h = 0.0f;
        c.keep = c.nsave = 0;
    }
}

// R64 dot of the window (lane-strided, registers) with a twiddle row.
template <int WPL>
__device__ __forceinline__ double window_dot(const double (&x)[WPL], const double* tab, int W) {
    const int lane = threadIdx.x & 63;
    double a = 0.0;
#pragma unroll
    for (int m = 0; m < WPL; ++m) {
        const int i = lane + 64 * m;
        if (i < W) a = __builtin_fma(x[m], tab[i], a);
    }
    return wave_sum_f64(a);
}

// Window accessor: x[i] (oldest first) of the window after this step's
// append is either an untouched slot of the ring or one of the S new samples
// held in LDS.
struct WinView {
    const double* ring;
    int e;
    int W, wp0, S;
    __device__ __forceinline__ double at(int i) const {
        const int keep = W - S;
        if (i < keep) {
            int k = wp0 + S + i;
            if (k >= W) k -= W;
            return ring[k];
        }
        return s_smp_r[e][i - keep];
    }
};

// Reward of the window held in registers (R64 layout), env.py:638-688 (the
// standalone reward kernel).  Must be called by the whole wave.
//   R1 / R3: the 10 beta bins as float64 DFT dots (calc_beta_band_power,
//            utils.py:21-27);
//   R2:      d = c . x, the filtfilt term as a linear functional (kura_r2.h:
//            f[-1] - mean(f) of scipy's filtfilt is linear in the window).
template <int WPL>
__device__ __forceinline__ double reward_of(DevParamsK& p, const double (&x)[WPL], double u0) {
    const double au = fabs(u0);
    if (p.reward_kind == KURA_R_TEMP_CONST) {
        const double d = window_dot<WPL>(x, p.r2c, p.W);
        const double r1 = 1e3 * (d * d);
        return -r1 - 1e-2 * au;
    }
    double bb = 0.0;
    for (int b = 0; b < p.n_bins; ++b) {
        const double re = window_dot<WPL>(x, p.ctab + (size_t)b * p.W, p.W);
        const double im = window_dot<WPL>(x, p.stab + (size_t)b * p.W, p.W);
        const double pr = re / (double)p.W, pi = im / (double)p.W;
        const double pw = (pr * pr + pi * pi) * 2.0;
        bb = bb + pw;
    }
    if (p.reward_kind == KURA_R_BBPOW_THR) {
        const double bs = 1e4 * bb;
        const double r1 = bs > 20.0 ? 5.0 : 0.0;
        return -r1 - au;
    }
    const double r1 = 1e4 * bb;
    return -r1 - 1e-2 * au;
}

#define WPL_MAX 40  // ceil(W/64) upper bound supported (W <= 2560)

// R2's filter term d = c . x (kura_r2.h) of the windows of NE envs of one
// wave at once, in the R64 order of window_dot (lane l accumulates
// x[l + 64 m] * c[l + 64 m] over m from +0 by fma, then the xor butterfly):
// one W-long dot per env in place of scipy's two serial filtfilt passes.  c
// is read once per element for all NE envs (buffer loads through one
// wave-uniform descriptor), the windows straight from the ring / this step's
// samples (WinView).  ok[e] false: d[e] = 0 and nothing of env e is read.
template <int NE>
__device__ __forceinline__ void r2_dot_multi(DevParamsK& __restrict__ p, const WinView (&xv)[NE],
                                             const bool (&ok)[NE], double (&d)[NE]) {
    const int lane = threadIdx.x & 63;
    const int W = p.W;
    const int nm = (W + 63) / 64;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)uniform_ptr(p.r2c), 0, W * 8,
                                                                      0x00020000);
    double acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.0;
#pragma unroll 4
    for (int m = 0; m < nm; ++m) {
        const int i = lane + 64 * m;
        const bool valid = i < W;
        const double c = __builtin_bit_cast(
            double, __builtin_amdgcn_raw_buffer_load_b64(rc, valid ? i * 8 : 0x7FFFFFF0, 0, 0));  // out of range: 0
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double x = (valid && ok[e]) ? xv[e].at(i) : 0.0;
            acc[e] = valid ? __builtin_fma(x, c, acc[e]) : acc[e];
        }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) d[e] = ok[e] ? wave_sum_f64(acc[e]) : 0.0;
}

// ---- R1 / R3 beta power from running spectral accumulators ---------------
// calc_beta_band_power (utils.py:21-27) needs |X_k|^2 of the window's DFT at
// the 10 in-band bins k.  With the window kept as a ring, X_k of the window
// (oldest first) is e^{2 pi i k wpos / W} times Y_k = sum_p ring[p] e^{-2 pi i
// k p / W}, the DFT over ring positions -- a pure phase, so |X_k| = |Y_k|.
// Y_k changes only at the S slots a step overwrites:
//     Y_k += (new - old) * (cos, -sin)(2 pi k p / W)    for each written slot p,
// so each env keeps Y (spec[env][2 n_bins]: re, im per bin, float64) and a
// step costs S * 2 n_bins fmas instead of 2 n_bins W-long dots.  The reset
// (and kura_set_state / kura_set_spec) forms Y directly (spec_init, R64
// order); the oracle keeps the same accumulators with the same operations
// (oracle/kura_oracle.c spec_update), so the reward stays bit-exact, and it
// agrees with the direct DFT to float64 rounding: over a whole 5555-step
// episode 2.2e-14 relative on the band power and 8.6e-15 of sum|x| on Y_k
// (tests/test_r2_functional.py::test_accumulators_hold_over_a_whole_episode,
// bound 1e-12).

// whole wave: Y of env `env` from its ring (positions 0..W-1), R64 dots
__device__ __forceinline__ void spec_init(DevParamsK& __restrict__ p, int env) {
    const int lane = threadIdx.x & 63;
    const int W = p.W, nb = p.n_bins;
    const double* rb = p.ring + (size_t)env * W;
    double* sp = p.spec + (size_t)env * 2 * nb;
    for (int b = 0; b < nb; ++b) {
        double re = 0.0, im = 0.0;
        for (int i = lane; i < W; i += 64) {
            const double x = rb[i];
            re = __builtin_fma(x, p.ctab[(size_t)b * W + i], re);
            im = __builtin_fma(x, p.stab[(size_t)b * W + i], im);
        }
        re = wave_sum_f64(re);
        im = wave_sum_f64(im);
        if (lane == 0) {
            sp[2 * b] = re;
            sp[2 * b + 1] = im;
        }
    }
}

// whole wave, before the ring append of env `env` (local env e): fold this
// step's S samples (LDS s_smp_r[e]) into Y in sample order and return the
// band power of the new window (the bins summed in index order from +0, as
// calc_beta_band_power's np.sum does in the oracle).  Lane j < 2 n_bins owns
// Y's component j (bin j/2, re or im) and walks the S slots in order.
__device__ __forceinline__ double spec_step(DevParamsK& __restrict__ p, int e, int env, int wp0, int S) {
    const int lane = threadIdx.x & 63;
    const int W = p.W, nb = p.n_bins;
    // the values the S appends overwrite, read before any of them is stored
    // (lane s; a slot written twice in one step, S > W, sees the first append)
    double oldv = 0.0;
    if (lane < S) {
        int k = wp0 + lane;
        while (k >= W) k -= W;
        oldv = lane >= W ? s_smp_r[e][lane - W] : p.ring[(size_t)env * W + k];
    }
    double* sp = p.spec + (size_t)env * 2 * nb;
    const bool own = lane < 2 * nb;
    const double* tab = ((lane & 1) ? p.stab : p.ctab) + (size_t)(lane >> 1) * W;
    double acc = own ? sp[lane] : 0.0;
    int k = wp0;
    for (int s = 0; s < S; ++s) {   // S is uniform over the wave
        const double od = __shfl(oldv, s, 64);
        const double dl = s_smp_r[e][s] - od;
        if (own) acc = __builtin_fma(dl, tab[k], acc);
        k = k + 1 == W ? 0 : k + 1;
    }
    if (own) sp[lane] = acc;
    double bb = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double re = __shfl(acc, 2 * b, 64), im = __shfl(acc, 2 * b + 1, 64);
        const double pr = re / (double)W, pi = im / (double)W;
        bb = bb + (pr * pr + pi * pi) * 2.0;
    }
    return bb;
}

// reward_of's closing expressions (env.py:638-688) from the band power bb (R1,
// R3) or the filter term d (R2)
__device__ __forceinline__ double reward_from(DevParamsK& p, double bb, double d, double u0) {
    const double au = fabs(u0);
    if (p.reward_kind == KURA_R_TEMP_CONST) {
        const double r1 = 1e3 * (d * d);
        return -r1 - 1e-2 * au;
    }
    if (p.reward_kind == KURA_R_BBPOW_THR) {
        const double bs = 1e4 * bb;
        const double r1 = bs > 20.0 ? 5.0 : 0.0;
        return -r1 - au;
    }
    const double r1 = 1e4 * bb;
    return -r1 - 1e-2 * au;
}

// ------------------------------------------------------------ step kernel --
// Work item of a launch: (env group, part).  For N <= 1024 one workgroup per
// group; split groups loop persistently over pairs with a grid that is a
// multiple of npart and at most one workgroup per CU, so every part of a
// group is resident at the same time.
__device__ __forceinline__ Part make_part(DevParamsK& p, int pair) {
    Part pt;
    pt.npart = p.npart;
    pt.group = pair / p.npart;
    pt.part = pair - pt.group * p.npart;
    pt.ng = p.N;
    pt.col0 = pt.part * (p.N / p.npart);
    pt.pair = pair;
    pt.ep = 0;
    pt.xs_n = 0;
    return pt;
}

// Launch-wide failure bits an env inherits: a split-group barrier that timed
// out (group_barrier) leaves every later exchange of the launch unsynchronised.
__device__ __forceinline__ int launch_flags(DevParamsK& p, bool xl) {
    if (!xl) return 0;  // split groups only: their group barriers can time out
    const unsigned long long v = __hip_atomic_load((__attribute__((address_space(1))) unsigned long long*)&p.stats[3],
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (int)(v & KURA_F_BARRIER);
}

template <int TPW, bool XL, bool SP>
__device__ __forceinline__ void step_pair(DevParamsK& p, Part& pt, float* Xs, const float* __restrict__ action,
                                          float* __restrict__ obs, double* __restrict__ reward,
                                          uint8_t* __restrict__ done, float* __restrict__ lfp_true,
                                          double* __restrict__ lfp_rec, int* __restrict__ nsamp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int N = p.N;
    const int env_base = pt.group * E_WG;
    const int c0 = XL ? pt.col0 : 0, c1 = XL ? pt.col0 + TPW * 256 : N;   // oscillators of this workgroup
    __syncthreads();  // previous pair's LDS readers
    ctl_clear();
    // ---- thread e: rescale_action (env.py:389-393), ON grid (env.py:426-428)
    if (tid < E_WG) {
        const int env = env_base + tid;
        s_nI[tid] = s_nII[tid] = 0;
        for (int k = 0; k < 4; ++k) s_u[tid][k] = 0.0;
        if (env < p.B) {
            const int ne = p.n_elec < 4 ? p.n_elec : 4;
            for (int k = 0; k < ne; ++k) {
                const double a = (double)action[(size_t)env * p.n_elec + k];
                s_u[tid][k] = p.dbs_lo + ((p.dbs_hi - p.dbs_lo) * (a - p.act_lo)) / (p.act_hi - p.act_lo);
            }
            const double t = p.t[env];
            const Grid g = make_grid(t, t + p.width, p.dt);
            s_nI[tid] = g.n;
            ctl_begin(s_ctl[tid], g, p.dt0, 0, g.n, 0);
            if (g.n < 2 || g.n > KURA_S_MAX) {
                s_ctl[tid].active = 0;
                s_ctl[tid].flags |= KURA_F_GRID;
            }
        }
    }
    __syncthreads();
    // ---- pulse = float32(sum_e g_e * u_e) for the envs of this wave (env.py:419-424)
#pragma unroll 1
    for (int ee = 0; ee < ENVS_PER_WAVE; ++ee) {
        const int e = wave * ENVS_PER_WAVE + ee;
        const int env = env_base + e;
        if (env >= p.B) continue;
        const int ne = p.n_elec < 4 ? p.n_elec : 4;
        for (int i = c0 + lane; i < c1; i += 64) {
            double pacc = 0.0;
            for (int k = 0; k < ne; ++k) pacc = pacc + p.g_stim[((size_t)env * p.n_elec + k) * N + i] * s_u[e][k];
            p.pulse[(size_t)env * N + i] = (float)pacc;
        }
    }
    __syncthreads();
    long long rhs = 0;
    // the stim-ON solve, then the stim-OFF solve: one call site of the
    // (inlined) solver, so the kernel carries no call frame for it
#pragma unroll 1
    for (int ph = 0; ph < 2; ++ph) {
        if (ph == 1) {
            __syncthreads();  // global stores of the solve (y) before the OFF setup
            // ---- stimulation OFF (env.py:433-441)
            if (tid < E_WG) {
                CtlE& c = s_ctl[tid];
                const int env = env_base + tid;
                c.active = 0;
                if (env < p.B && !c.flags) {
                    const int nI = s_nI[tid];
                    const double tm = grid_at_c(c, nI - 1);
                    const Grid g = make_grid(tm, tm + p.pause, p.dt);
                    s_nII[tid] = g.n;
                    ctl_begin(c, g, p.dt0, 1, g.n - 1, nI + 1);
                    if (g.n < 2 || nI + g.n - 1 > KURA_S_MAX) {
                        c.active = 0;
                        c.flags |= KURA_F_GRID;
                    } else {  // ys_II[0] == ys_I[-1]: duplicated sample (env.py:440)
                        s_smp_n[tid][nI] = s_smp_n[tid][nI - 1];
                        s_smp_r[tid][nI] = s_smp_r[tid][nI - 1];
                    }
                }
            }
            __syncthreads();
        }
        solve_wg<TPW, XL, SP, false>(p, Xs, env_base, ph == 0, &rhs, pt);
    }
    STAMP_DECL  // diagnostic build: the tail's phases in slots 20-22
    __syncthreads();
    // ---- window, reward, outputs (env.py:443-454): wave w owns envs 2w, 2w+1
    // (split groups: part 0; every part holds the same samples)
    // R2: d = c . x of both envs of the wave at once (r2_dot_multi), before
    // the ring appends below overwrite the window's oldest slots
    double r2d[ENVS_PER_WAVE] = {0.0, 0.0};
    const bool r2 = p.reward_kind == KURA_R_TEMP_CONST;
    if (r2 && (!XL || pt.part == 0)) {
        WinView xvs[ENVS_PER_WAVE];
        bool oks[ENVS_PER_WAVE];
#pragma unroll
        for (int ee = 0; ee < ENVS_PER_WAVE; ++ee) {
            const int e = wave * ENVS_PER_WAVE + ee;
            const int env = env_base + e;
            const int S = s_nI[e] + s_nII[e] - 1;
            oks[ee] = env < p.B && !(s_ctl[e].flags | launch_flags(p, XL)) && S >= 1;
            xvs[ee] = WinView{p.ring + (size_t)(oks[ee] ? env : 0) * p.W, e, p.W, oks[ee] ? p.wpos[env] : 0, S};
        }
        r2_dot_multi<ENVS_PER_WAVE>(p, xvs, oks, r2d);
    }
    STAMP(21);
#pragma unroll 1
    for (int ee = 0; ee < ((!XL || pt.part == 0) ? ENVS_PER_WAVE : 0); ++ee) {
        const int e = wave * ENVS_PER_WAVE + ee;
        const int env = env_base + e;
        if (env >= p.B) continue;
        const CtlE& c = s_ctl[e];
        const int S = s_nI[e] + s_nII[e] - 1;
        const int fl = c.flags | launch_flags(p, XL);
        if (lane == 0) p.eflags[env] = fl;
        if (fl || S < 1) {
            // failed step (kura.h KURA_F_*): no state advance, done = 1; the
            // host raises (diffrax's throw=True) or resets the env
            if (lane == 0) {
                if (nsamp) nsamp[env] = 0;
                if (done) done[env] = 1;
                if (reward) reward[env] = 0.0;
            }
            continue;
        }
        const int W = p.W;
        double* rb = p.ring + (size_t)env * W;
        const int wp0 = p.wpos[env];
        STAMP(22);
        if (obs) {  // the new window, oldest first: 8 loads in flight per lane, then 8 stores
            float* __restrict__ ob = obs + (size_t)env * W;
            const double* __restrict__ rr = rb;
            const int keep = W - S;
#pragma unroll 1
            for (int i0 = 0; i0 < W; i0 += 64 * 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + lane + 64 * u;
                    const int ii = i < keep ? i : 0;       // ring slot of an untouched sample (in range)
                    int k = wp0 + S + ii;
                    if (k >= W) k -= W;
                    const double r = rr[k];
                    const int j = i < keep ? 0 : (i < W ? i : W - 1) - keep;   // this step's sample (in range)
                    double l = s_smp_r[e][j];
                    // two loads and a select of values: folded into one load through a selected
                    // generic pointer, ROCm 7.2's backend fails to select the LDS-aperture check
                    asm volatile("" : "+v"(l));
                    v[u] = i < keep ? r : l;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + lane + 64 * u;
                    if (i < W) ob[i] = (float)v[u];
                }
            }
        }
#ifdef KURA_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        STAMP(20);
        // R1 / R3: fold the S new samples into the env's spectral accumulators
        // (old slot values read before the append below) -> band power
        const double bb = r2 ? 0.0 : spec_step(p, e, env, wp0, S);
        const double r = reward_from(p, bb, r2d[ee], s_u[e][0]);
        // ring append after every read of the old slots
        if (lane < S) {
            int k = wp0 + lane;
            if (k >= W) k -= W;
            rb[k] = s_smp_r[e][lane];
        }
        int wp = wp0 + S;
        if (wp >= W) wp -= W;
        if (lane == 0) {
            p.wpos[env] = wp;
            const int st = p.step[env] + 1;
            p.step[env] = st;
            p.t[env] = grid_at_c(c, s_nII[e] - 1);
            if (reward) reward[env] = r;
            if (done) done[env] = st >= p.episode_steps;
            if (nsamp) nsamp[env] = S;
        }
        if (lane < KURA_S_MAX) {
            if (lfp_true) lfp_true[(size_t)env * KURA_S_MAX + lane] = lane < S ? s_smp_n[e][lane] : 0.0f;
            if (lfp_rec) lfp_rec[(size_t)env * KURA_S_MAX + lane] = lane < S ? s_smp_r[e][lane] : 0.0;
        }
        if (p.ep_lfp) {  // episode record: theta_mean of every step (evaluate_HF_DBS.py:83)
            const int L0 = p.ep_len[env];
            if (lane < S && L0 + lane < p.episode_cap)
                p.ep_lfp[(size_t)env * p.episode_cap + L0 + lane] = s_smp_n[e][lane];
            if (lane == 0) p.ep_len[env] = L0 + S;
        }
    }
    STAMP(22);
    STAMP_FLUSH(p);
    if (!XL || pt.part == 0) flush_stats(p, rhs, env_base);
}

// Split groups call the step body out of line.  Inlined into the persistent
// pair loop, the TPW = 1 split instantiation (parts of 256) came out of
// ROCm 7.2's compiler with one env slot of every lane (q = 4) integrated
// wrongly -- deterministic, gone at -O3 with this call boundary, present at
// -O2 as well (tools/parity_probe.py, profiles/r02_part256_probe.txt); the
// GPU parity suite covers every instantiation.
template <int TPW, bool XL, bool SP>
__device__ __noinline__ void step_pair_call(DevParamsK& pin, Part& pt, float* Xs, const float* __restrict__ action,
                                            float* __restrict__ obs, double* __restrict__ reward,
                                            uint8_t* __restrict__ done, float* __restrict__ lfp_true,
                                            double* __restrict__ lfp_rec, int* __restrict__ nsamp) {
    step_pair<TPW, XL, SP>(pin, pt, Xs, action, obs, reward, done, lfp_true, lfp_rec, nsamp);
}

template <int TPW, bool XL, bool SP>
__global__ __launch_bounds__(NTHREADS) void kura_step_kernel(DevParams p_kernarg, const float* __restrict__ action,
                                                             float* __restrict__ obs, double* __restrict__ reward,
                                                             uint8_t* __restrict__ done, float* __restrict__ lfp_true,
                                                             double* __restrict__ lfp_rec, int* __restrict__ nsamp) {
    DevParamsK& p = kargs();  // == p_kernarg, read in place (kernarg offset 0)
    (void)p_kernarg;
    extern __shared__ float Xs[];  // xs_floats(min(N, 1024))
    if constexpr (XL) {
#pragma unroll 1
        for (int pair = blockIdx.x; pair < p.npairs; pair += gridDim.x) {
            Part pt = make_part(p, pair);
            step_pair_call<TPW, XL, SP>(p, pt, Xs, action, obs, reward, done, lfp_true, lfp_rec, nsamp);
        }
    } else {
        Part pt = make_part(p, blockIdx.x);
        step_pair<TPW, XL, SP>(p, pt, Xs, action, obs, reward, done, lfp_true, lfp_rec, nsamp);
    }
}

// ----------------------------------------------------------- reset kernel --
template <int TPW, bool XL, bool SP>
__device__ __forceinline__ void reset_pair(DevParamsK& p, Part& pt, float* Xs, const uint8_t* __restrict__ mask,
                                           const float* __restrict__ theta0, float* __restrict__ obs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int N = p.N, W = p.W;
    const int env_base = pt.group * E_WG;
    const int c0 = XL ? pt.col0 : 0, c1 = XL ? pt.col0 + TPW * 256 : N;
    __syncthreads();
    ctl_clear();
    if (tid < E_WG) {
        const int env = env_base + tid;
        if (env < p.B && (!mask || mask[env])) {
            const Grid g = make_grid(0.0, p.transient_len, p.dt);
            ctl_begin(s_ctl[tid], g, p.dt0, p.lfp_tr ? 0 : g.n - 1 - W, g.n - 1, 0);
        }
    }
    // state y <- theta0 for the masked envs
#pragma unroll 1
    for (int ee = 0; ee < ENVS_PER_WAVE; ++ee) {
        const int env = env_base + wave * ENVS_PER_WAVE + ee;
        if (env >= p.B || (mask && !mask[env])) continue;
        for (int i = c0 + lane; i < c1; i += 64) p.y[(size_t)env * N + i] = theta0[(size_t)env * N + i];
    }
    __syncthreads();
    long long rhs = 0;
    solve_wg<TPW, XL, SP, true>(p, Xs, env_base, false, &rhs, pt);
    __syncthreads();  // ring rows written by thread e are read by every lane below
#pragma unroll 1
    for (int ee = 0; ee < ((!XL || pt.part == 0) ? ENVS_PER_WAVE : 0); ++ee) {
        const int e = wave * ENVS_PER_WAVE + ee;
        const int env = env_base + e;
        if (env >= p.B || (mask && !mask[env])) continue;
        if (lane == 0) {
            p.eflags[env] = s_ctl[e].flags | launch_flags(p, XL);
            p.t[env] = grid_at_c(s_ctl[e], s_ctl[e].n - 1);
            p.step[env] = 0;
            p.wpos[env] = 0;
            if (p.ep_len) p.ep_len[env] = 0;  // a new episode starts
        }
        if (obs)
            for (int i = lane; i < W; i += 64) obs[(size_t)env * W + i] = (float)p.ring[(size_t)env * W + i];
        // R1 / R3: the spectral accumulators of the new window (spec_step)
        if (p.reward_kind != KURA_R_TEMP_CONST) spec_init(p, env);
    }
    if (!XL || pt.part == 0) flush_stats(p, rhs, env_base);
}

// kura_set_state / kura_set_spec(NULL) / kura_set_spectral: re-form every
// env's spectral accumulators from its ring (one wave per env)
__global__ __launch_bounds__(64) void kura_spec_init_kernel(DevParams p_kernarg) {
    DevParamsK& p = kargs();  // == p_kernarg, read in place (kernarg offset 0)
    (void)p_kernarg;
    if ((int)blockIdx.x < p.B) spec_init(p, blockIdx.x);
}

template <int TPW, bool XL, bool SP>
__global__ __launch_bounds__(NTHREADS) void kura_reset_kernel(DevParams p_kernarg, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ theta0,
                                                              float* __restrict__ obs) {
    DevParamsK& p = kargs();  // == p_kernarg, read in place (kernarg offset 0)
    (void)p_kernarg;
    extern __shared__ float Xs[];
    if constexpr (XL) {
#pragma unroll 1
        for (int pair = blockIdx.x; pair < p.npairs; pair += gridDim.x) {
            Part pt = make_part(p, pair);
            reset_pair<TPW, XL, SP>(p, pt, Xs, mask, theta0, obs);
        }
    } else {
        Part pt = make_part(p, blockIdx.x);
        reset_pair<TPW, XL, SP>(p, pt, Xs, mask, theta0, obs);
    }
}

// ------------------------------------------------------ standalone reward --
template <int WPL>
__global__ __launch_bounds__(64) void kura_reward_kernel(DevParams p_kernarg, const double* __restrict__ win,
                                                         const float* __restrict__ u0, double* __restrict__ out,
                                                         int n) {
    DevParamsK& p = kargs();  // == p_kernarg, read in place (kernarg offset 0)
    (void)p_kernarg;
    const int env = blockIdx.x;
    if (env >= n) return;
    const int lane = threadIdx.x;
    const double* xl = win + (size_t)env * p.W;
    double x[WPL];
#pragma unroll
    for (int m = 0; m < WPL; ++m) {
        const int i = lane + 64 * m;
        x[m] = i < p.W ? xl[i] : 0.0;
    }
    const double r = reward_of<WPL>(p, x, (double)u0[env]);
    if (lane == 0) out[env] = r;
}

// ------------------------------------------- reward on any window length --
// reward_* of env.py:638-688 on 1-D windows of any length L (the reference
// computes the beta bins from len(x_state), utils.py:21-27, e.g. the n_envs*W
// samples PIDController.predict passes, aDBS_RL/agents/simple_dbs.py:81-88).
// One wave per window, read from memory: R1/R3 = the bins' R64 dots against
// host twiddle rows of length L (the same R64 order as window_dot, so a
// length-W call equals kura_reward bit for bit), R2 = the R64 dot with the
// length-L functional c (kura_r2.h; the host caches one per length).
__global__ __launch_bounds__(64) void kura_reward_n_kernel(DevParams p_kernarg, const double* __restrict__ x, long long ld,
                                                           const double* __restrict__ ctab,
                                                           const double* __restrict__ stab, int n_bins,
                                                           const double* __restrict__ u0, double* __restrict__ out,
                                                           const double* __restrict__ r2c, int n) {
    DevParamsK& p = kargs();  // == p_kernarg, read in place (kernarg offset 0)
    (void)p_kernarg;
    const int j = blockIdx.x;
    if (j >= n) return;
    const int lane = threadIdx.x;
    const int L = p.W;
    const double* xw = x + (size_t)j * ld;
    const double au = fabs(u0[j]);  // float64: the caller's action as given (env.py:638-688)
    double r;
    if (p.reward_kind == KURA_R_TEMP_CONST) {
        double d = 0.0;
        for (int i = lane; i < L; i += 64) d = __builtin_fma(xw[i], r2c[i], d);
        d = wave_sum_f64(d);
        r = -(1e3 * (d * d)) - 1e-2 * au;
    } else {
        double bb = 0.0;
        for (int b = 0; b < n_bins; ++b) {
            double re = 0.0, im = 0.0;
            for (int i = lane; i < L; i += 64) {
                re = __builtin_fma(xw[i], ctab[(size_t)b * L + i], re);
                im = __builtin_fma(xw[i], stab[(size_t)b * L + i], im);
            }
            re = wave_sum_f64(re);
            im = wave_sum_f64(im);
            const double pr = re / (double)L, pi = im / (double)L;
            bb = bb + (pr * pr + pi * pi) * 2.0;
        }
        if (p.reward_kind == KURA_R_BBPOW_THR) {
            r = -(1e4 * bb > 20.0 ? 5.0 : 0.0) - au;
        } else {
            r = -(1e4 * bb) - 1e-2 * au;
        }
    }
    if (lane == 0) out[j] = r;
}

#include "kura_fft.inc"

// ------------------------------------------------------------- self-tests --
#define KURA_SELFTEST_MATH_W 10
__global__ void kura_selftest_math_kernel(const float* x, const float* y, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* o = out + (size_t)i * KURA_SELFTEST_MATH_W;
    float s, c;
    kdm_sincosf(x[i], &s, &c);
    o[0] = s;
    o[1] = c;
    o[2] = kdm_fmod2pi(x[i]);
    o[3] = kdm_inv_fifth_root(fabsf(y[i]));
    o[4] = sqrtf(fabsf(x[i]));
    o[5] = x[i] / y[i];
    o[6] = (float)((double)x[i] / (double)y[i]);
    o[7] = (float)ceil((double)x[i] / 0.05);
    kdm_sincos_fmod2pi(x[i], &s, &c);   // the RHS's theta = fmod(y, 2pi_f) -> sin, cos
    o[8] = s;
    o[9] = c;
}

// One 32-row coupling GEMM through the production GEMM path.
template <int TPW, bool SP>
__global__ __launch_bounds__(NTHREADS) void kura_selftest_gemm_kernel(const float* X, const float* alpha_sw,
                                                                       float* Y, int N, int reuse) {
    extern __shared__ float Xs[];
    for (int idx = threadIdx.x; idx < 32 * N; idx += blockDim.x) {
        const int r = idx / N, k = idx % N;
        Xs[xs_idx(r, k)] = X[idx];
    }
    __syncthreads();
    floatx16 acc[TPW];
    coupling_gemm<TPW, SP>(Xs, alpha_sw, reuse, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
            const int col = 32 * (wave * TPW + t) + (lane & 31);
            Y[(size_t)row * N + col] = acc[t][q];
        }
}

#include "kura_capi.inc"
