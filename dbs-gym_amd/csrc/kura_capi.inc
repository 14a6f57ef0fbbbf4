// kura_capi.inc -- host side of libkura: the handle, validation, launchers and
// the extern "C" entry points declared in include/kura.h.  Included at the end
// of kura_kernels.hip so the kernel templates are instantiated in one TU.
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "kura_r2.h"

namespace {

thread_local char g_err[512] = "";

int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return set_err(KURA_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

template <class T>
int dalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return set_err(KURA_E_NOMEM, "hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(e));
    (void)hipMemset(*p, 0, n * sizeof(T));
    return KURA_OK;
}

}  // namespace

#define R2C_CACHE 4   // kura_reward_n: R2 functionals kept per handle (most recently used lengths)

struct KuraHandle {
    KuraConfig cfg;
    int device;
    int B;
    int tpw;
    bool xl = false;      // split groups (N > 1024)
    bool sp = false;      // KURA_COUPLING_BF16X3 (kura_coupling_of)
    bool xl_plain = false;  // KURA_XL_LAUNCH=plain: split groups by hipLaunchKernel (launch_xl)
    int ncu = 256;        // compute units (co-residency bound of split-group launches)
    int ngroups = 0;
    DevParams p;
    bool have_coupling = false, have_params = false, have_spectral = false, was_reset = false;
    float* alpha_sw = nullptr;
    size_t alpha_cap = 0;           // floats allocated at alpha_sw
    float* alpha_dd = nullptr;      // BF16X3, N <= 1024: the deduplicated image (the reset's GEMM)
    size_t alpha_dd_cap = 0;
    float* omega = nullptr;
    float* kn_env = nullptr;
    double* g_stim = nullptr;
    double* g_rec = nullptr;
    double* ctab = nullptr;
    double* stab = nullptr;
    float* y = nullptr;
    double* t = nullptr;
    int* step = nullptr;
    double* ring = nullptr;
    int* wpos = nullptr;
    float* R = nullptr;
    float* pulse = nullptr;
    double* r2c = nullptr;          // [W] R2 filter functional (kura_r2.h)
    double* spec = nullptr;         // [Bp][2 n_bins] R1/R3 spectral accumulators
    std::vector<std::pair<long long, double*>> r2c_len;  // kura_reward_n: functional per window length (MRU first)
    unsigned long long* stats = nullptr;
    unsigned long long* stamps = nullptr;
    float* xg = nullptr;
    float* xred = nullptr;
    double* xredd = nullptr;
    unsigned* gcnt = nullptr;
    float* ep_lfp = nullptr;
    int* ep_len = nullptr;
    int* eflags = nullptr;          // [Bp] KURA_F_* of the last launch
    void* met_scratch = nullptr;    // episode-metric FFT / filter buffers (grown on demand)
    size_t met_scratch_n = 0;
};

static int validate(const KuraConfig* c) {
    if (!c) return set_err(KURA_E_INVALID, "null config");
    if (c->abi_version != KURA_ABI_VERSION)
        return set_err(KURA_E_INVALID, "abi_version %d != %d%s", c->abi_version, KURA_ABI_VERSION,
                       c->abi_version == 1 ? " (a version-1 config has no coupling field: choose "
                                             "KuraConfig.coupling and set abi_version = 2)" : "");
    if (c->n_osc != 256 && c->n_osc != 512 && c->n_osc != 1024 && c->n_osc != 2048 && c->n_osc != 4096 &&
        c->n_osc != 8192)
        return set_err(KURA_E_UNSUPPORTED, "n_osc=%d: this build supports N in {256, 512, ..., 8192}", c->n_osc);
    if (c->n_envs < 1) return set_err(KURA_E_INVALID, "n_envs=%d", c->n_envs);
    if (c->coupling < KURA_COUPLING_AUTO || c->coupling > KURA_COUPLING_BF16X3)
        return set_err(KURA_E_INVALID, "coupling=%d: expected KURA_COUPLING_AUTO, _F32 or _BF16X3", c->coupling);
    if (c->window < KURA_S_MAX || c->window > 64 * WPL_MAX)  // (a step's samples never wrap the ring twice)
        return set_err(KURA_E_UNSUPPORTED, "window=%d outside [%d, %d]", c->window, KURA_S_MAX, 64 * WPL_MAX);
    if (c->n_elec < 1 || c->n_elec > 4) return set_err(KURA_E_UNSUPPORTED, "n_elec=%d outside [1,4]", c->n_elec);
    if (c->episode_cap < 0) return set_err(KURA_E_INVALID, "episode_cap=%d", c->episode_cap);
    if (c->n_rec < 0 || c->n_rec > 4) return set_err(KURA_E_UNSUPPORTED, "n_rec=%d outside [0,4]", c->n_rec);
    if (c->rec_kernel != KURA_REC_NAIVE && c->rec_kernel != KURA_REC_GAUSSIAN)
        return set_err(KURA_E_INVALID, "Wrong recording kernel function! (%d)", c->rec_kernel);
    if (c->rec_kernel == KURA_REC_GAUSSIAN && c->n_rec < 1)
        return set_err(KURA_E_INVALID, "gaussian recording kernel needs n_rec >= 1");
    if (c->reward_kind < 1 || c->reward_kind > 3) return set_err(KURA_E_INVALID, "Wrong reward function! (%d)", c->reward_kind);
    if (c->n_bins < 0 || c->n_bins > KURA_MAX_BINS) return set_err(KURA_E_INVALID, "n_bins=%d", c->n_bins);
    for (int b = 0; b < c->n_bins; ++b)
        if (c->bins[b] < 0 || c->bins[b] > c->window / 2) return set_err(KURA_E_INVALID, "bin %d out of range", c->bins[b]);
    if (c->reward_kind == KURA_R_TEMP_CONST && (c->padlen < 1 || c->padlen >= c->window))
        return set_err(KURA_E_INVALID, "padlen=%d", c->padlen);
    if (!(c->dt > 0) || !(c->width > 0) || !(c->pause > 0) || !(c->transient_len > 0))
        return set_err(KURA_E_INVALID, "dt/width/pause/transient_len must be > 0");
    double ntr = ceil(c->transient_len / c->dt);
    if (ntr - 1 < c->window)
        return set_err(KURA_E_INVALID, "Transient state should be longer than RL agent observation window!");
    if (c->max_steps < 1) return set_err(KURA_E_INVALID, "max_steps=%d", c->max_steps);
    if (!(c->dt0 > 0) || !(c->rtol >= 0) || !(c->atol >= 0)) return set_err(KURA_E_INVALID, "dt0/rtol/atol");
    return KURA_OK;
}

static void fill_params(KuraHandle* h) {
    const KuraConfig& c = h->cfg;
    DevParams& p = h->p;
    p.N = c.n_osc;
    p.B = c.n_envs;
    p.W = c.window;
    p.n_elec = c.n_elec;
    p.n_rec = c.n_rec;
    p.rec_kernel = c.rec_kernel;
    p.reward_kind = c.reward_kind;
    p.episode_steps = c.episode_steps;
    p.max_steps = c.max_steps;
    p.n_bins = c.n_bins;
    p.padlen = c.padlen;
    for (int i = 0; i < KURA_MAX_BINS; ++i) p.bins[i] = c.bins[i];
    p.dt = c.dt;
    p.width = c.width;
    p.pause = c.pause;
    p.transient_len = c.transient_len;
    p.act_lo = c.act_lo;
    p.act_hi = c.act_hi;
    p.dbs_lo = c.dbs_lo;
    p.dbs_hi = c.dbs_hi;
    for (int i = 0; i < 5; ++i) { p.bw_b[i] = c.bw_b[i]; p.bw_a[i] = c.bw_a[i]; }
    for (int i = 0; i < 4; ++i) p.bw_zi[i] = c.bw_zi[i];
    p.rtol = c.rtol;
    p.atol = c.atol;
    p.kn = c.kn;
    p.dt0 = c.dt0;
    p.alpha_sw = h->alpha_sw;
    p.alpha_dd = h->alpha_dd;
    p.alpha_dd_bytes = (unsigned)(h->alpha_dd_cap * sizeof(float));
    p.alpha_reuse = 0;   // kura_set_coupling decides
    p.omega = h->omega;
    p.kn_env = h->kn_env;
    p.g_stim = h->g_stim;
    p.g_rec = h->g_rec;
    p.ctab = h->ctab;
    p.stab = h->stab;
    p.y = h->y;
    p.t = h->t;
    p.step = h->step;
    p.ring = h->ring;
    p.wpos = h->wpos;
    p.R = h->R;
    p.pulse = h->pulse;
    p.r2c = h->r2c;
    p.spec = h->spec;
    p.stats = h->stats;
    p.stamps = h->stamps;
    p.npart = h->xl ? c.n_osc / (h->tpw * 256) : 1;
    p.npairs = h->ngroups * p.npart;
    p.xg = h->xg;
    p.xred = h->xred;
    p.xredd = h->xredd;
    p.gcnt = h->gcnt;
    p.episode_cap = c.episode_cap;
    p.ep_lfp = h->ep_lfp;
    p.ep_len = h->ep_len;
    p.eflags = h->eflags;
    p.rows = nullptr;
    p.lfp_tr = nullptr;
    p.rows_tr = nullptr;
    p.n_tr = (int)ceil((c.transient_len - 0.0) / c.dt);   // make_grid(0, transient_len, dt).n
    p.gemm_dump = nullptr;
    p.gemm_dump_n = 0;
}

// Host swizzle of alpha into MFMA 32x32x2 B fragments:
//   sw[((jt*(N/8) + kb)*64 + lane)*4 + s] = alpha[32 jt + (lane&31)][8 kb + 2 s + (lane>>5)]
static void swizzle_alpha(const float* alpha, float* sw, int N) {
    const int NK8 = N / 8;
    for (int jt = 0; jt < N / 32; ++jt)
        for (int kb = 0; kb < NK8; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s) {
                    const int i = 32 * jt + (lane & 31);
                    const int k = 8 * kb + 2 * s + (lane >> 5);
                    sw[(((size_t)jt * NK8 + kb) * 64 + lane) * 4 + s] = alpha[(size_t)i * N + k];
                }
}

// KURA_COUPLING_BF16X3 (coupling_gemm_bf16x3): alpha as three bf16 parts (round to nearest even, exact residuals), per column tile
// jt, 16-deep k-block b, part p, lane l: 8 values at k = 16b + 8(i/4) +
// 2(i%4) + l/32, column 32 jt + l%32.
static uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static float bf16_f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// one B fragment (column tile jt, k-block b): 3 parts x 64 lanes x 8 bf16
static void split_fragment(const float* alpha, int N, int jt, int b, uint16_t* f) {
    for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 8; ++i) {
            const int col = 32 * jt + (lane & 31);
            const int k = 16 * b + 8 * (i / 4) + 2 * (i % 4) + (lane >> 5);
            const float a = alpha[(size_t)col * N + k];
            const uint16_t h1 = bf16_rne(a);
            const float r1 = a - bf16_f(h1);
            const uint16_t h2 = bf16_rne(r1);
            const uint16_t h3 = bf16_rne(r1 - bf16_f(h2));
            const uint16_t hp[3] = {h1, h2, h3};
            for (int p = 0; p < 3; ++p) f[(p * 64 + lane) * 8 + i] = hp[p];
        }
}
static void split_alpha(const float* alpha, uint16_t* sp, int N) {
    const int NB = N / 16;
    for (int jt = 0; jt < N / 32; ++jt)
        for (int b = 0; b < NB; ++b) split_fragment(alpha, N, jt, b, sp + ((size_t)jt * NB + b) * 3 * 64 * 8);
}

// Does the pre-split N = 1024 image (split_alpha) have the shift structure
// coupling_gemm_bf16x3_shift relies on?  Every fragment that form does not
// load -- column tile jt with jt % 4 != 0, k-block b with b % 8 >= 2, 1152 of
// 2048 -- must equal, byte for byte, the one it reuses: (jt - 1, b - 2).
// Pure host code; decided from the data on every kura_set_coupling.
static bool alpha_shift_reuse(const uint16_t* sp, int N) {
    if (N != 1024) return false;
    const int NB = N / 16;
    const size_t FU16 = 3 * 64 * 8;   // uint16 per fragment
    for (int jt = 0; jt < N / 32; ++jt)
        for (int b = 0; b < NB; ++b) {
            if (jt % 4 == 0 || b % 8 < 2) continue;
            if (memcmp(sp + ((size_t)jt * NB + b) * FU16, sp + ((size_t)(jt - 1) * NB + (b - 2)) * FU16, FU16 * 2))
                return false;
        }
    return true;
}
// KURA_ALPHA_REUSE=0 in the environment forces the general GEMM (tests, the
// same-binary A/B); read on every call.
static bool alpha_reuse_allowed() {
    const char* e = getenv("KURA_ALPHA_REUSE");
    return !(e && e[0] == '0' && e[1] == 0);
}

// alpha in the layout of the handle's coupling GEMM (floats of the image:
// N*N fp32 fragments, or N*N*3 bf16 parts).  BF16X3 reads pre-split parts,
// except split groups with parts of at most KURA_XL_SP_STAGED_MAXTPW * 256,
// whose GEMM splits the fp32 image in registers (coupling_gemm_xl_bf16x3).
static bool presplit_image(int N, bool sp, int tpw) {
    return sp && (N <= XL_NL || tpw > KURA_XL_SP_STAGED_MAXTPW);
}
// The pre-split BF16X3 image of split groups (coupling_gemm_xl_bf16x3_kb): a
// map [NB][N/32] of int32 byte offsets, then the distinct B fragments (3
// parts x 64 lanes x 16 B) in first-seen order; on the reference's
// grid-translation-invariant alpha 131072 fragments are 992 at N = 8192
// (3 MB instead of 403 MB).  (K1's step streams the plain image -- the
// scalar-loaded map cost it 7 %, profiles/r05_dedup_and_xl_forms_ab.txt --
// while K1's reset reads a second, deduplicated copy, h->alpha_dd: over the
// transient's 457 sweeps the plain image misses L2, r06_reset_dedup_ab.txt.)
// Each fragment is
// split on its own and looked up by a 64-bit FNV-1a hash, a match confirmed
// by memcmp; the device image is sized to the distinct fragments
// (kura_set_coupling).
static uint64_t fnv1a64(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}
static std::vector<float> split_alpha_dedup(const float* alpha, int N, int* nfrag = nullptr) {
    const int NB = N / 16, NT = N / 32;
    const size_t FU16 = 3 * 64 * 8;                          // uint16 per fragment
    const size_t MAPF = (size_t)NT * NB;                     // floats of the map
    std::vector<uint16_t> frags;                             // the distinct fragments, first-seen order
    std::vector<int32_t> map(MAPF);
    std::unordered_multimap<uint64_t, int> seen;
    std::vector<uint16_t> f(FU16);
    int n = 0;
    for (int jt = 0; jt < NT; ++jt)
        for (int b = 0; b < NB; ++b) {
            split_fragment(alpha, N, jt, b, f.data());
            const uint64_t key = fnv1a64(f.data(), FU16 * 2);
            int id = -1;
            for (auto r = seen.equal_range(key); r.first != r.second; ++r.first)
                if (!memcmp(frags.data() + (size_t)r.first->second * FU16, f.data(), FU16 * 2)) {
                    id = r.first->second;
                    break;
                }
            if (id < 0) {
                id = n++;
                seen.emplace(key, id);
                frags.insert(frags.end(), f.begin(), f.end());
            }
            map[(size_t)b * NT + jt] = (int32_t)(MAPF * 4 + (size_t)id * FU16 * 2);
        }
    if (nfrag) *nfrag = n;
    std::vector<float> img(MAPF + (size_t)n * FU16 / 2);
    memcpy(img.data(), map.data(), MAPF * 4);
    memcpy(img.data() + MAPF, frags.data(), (size_t)n * FU16 * 2);
    return img;
}
static std::vector<float> coupling_image(const float* alpha, int N, bool sp, int tpw) {
    if (presplit_image(N, sp, tpw) && N > XL_NL) return split_alpha_dedup(alpha, N);
    sp = presplit_image(N, sp, tpw);
    std::vector<float> sw(sp ? (size_t)N * N * 3 / 2 : (size_t)N * N);
    if (sp)
        split_alpha(alpha, reinterpret_cast<uint16_t*>(sw.data()), N);
    else
        swizzle_alpha(alpha, sw.data(), N);
    return sw;
}
// Floats kura_create allocates for the image; the deduplicated image (0 here)
// is allocated by kura_set_coupling at its actual size.
static size_t coupling_image_alloc(int N, bool sp, int tpw) {
    if (!presplit_image(N, sp, tpw)) return (size_t)N * N;
    return N > XL_NL ? 0 : (size_t)N * N * 3 / 2;
}

// dynamic LDS of a launch: the 32 x N operand, or (split groups) the two
// streamed chunk images of the XL GEMM, which also hold the part's own image
static size_t launch_lds(const KuraHandle* h) {
    return (size_t)(h->xl ? 2 * XL_CIMG : xs_floats(h->tpw * 256)) * sizeof(float);
}

// The step / reset kernels of a handle: (TPW, split groups, coupling).
template <int TPW, bool XL, bool SP>
static void kernels_of(const void** step, const void** reset) {
    *step = (const void*)kura_step_kernel<TPW, XL, SP>;
    *reset = (const void*)kura_reset_kernel<TPW, XL, SP>;
}

static int select_kernels(int tpw, bool xl, bool sp, const void** step, const void** reset) {
    switch ((tpw == 1 ? 0 : tpw == 2 ? 1 : 2) + 3 * (xl ? 1 : 0) + 6 * (sp ? 1 : 0)) {
        case 0: kernels_of<1, false, false>(step, reset); break;
        case 1: kernels_of<2, false, false>(step, reset); break;
        case 2: kernels_of<4, false, false>(step, reset); break;
        case 3: kernels_of<1, true, false>(step, reset); break;
        case 4: kernels_of<2, true, false>(step, reset); break;
        case 5: kernels_of<4, true, false>(step, reset); break;
        case 6: kernels_of<1, false, true>(step, reset); break;
        case 7: kernels_of<2, false, true>(step, reset); break;
        case 8: kernels_of<4, false, true>(step, reset); break;
        case 9: kernels_of<1, true, true>(step, reset); break;
        case 10: kernels_of<2, true, true>(step, reset); break;
        default: kernels_of<4, true, true>(step, reset); break;
    }
    return KURA_OK;
}

static const void* selftest_gemm_kernel(int tpw, bool sp) {
    switch ((tpw == 1 ? 0 : tpw == 2 ? 1 : 2) + 3 * (sp ? 1 : 0)) {
        case 0: return (const void*)kura_selftest_gemm_kernel<1, false>;
        case 1: return (const void*)kura_selftest_gemm_kernel<2, false>;
        case 2: return (const void*)kura_selftest_gemm_kernel<4, false>;
        case 3: return (const void*)kura_selftest_gemm_kernel<1, true>;
        case 4: return (const void*)kura_selftest_gemm_kernel<2, true>;
        default: return (const void*)kura_selftest_gemm_kernel<4, true>;
    }
}

static int prepare_kernels(int tpw, size_t lds, bool xl, bool sp) {
    const void *ks, *kr;
    int rc = select_kernels(tpw, xl, sp, &ks, &kr);
    if (rc) return rc;
    HIP_TRY(hipFuncSetAttribute(ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipFuncSetAttribute(kr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return KURA_OK;
}

// Launch of a kernel selected at run time (N <= 1024: one workgroup per env group).
template <typename... A>
static int launch_plain(const void* fn, dim3 grid, size_t lds, hipStream_t s, A... args) {
    void* argv[] = {(void*)&args...};
    HIP_TRY(hipLaunchKernel(fn, grid, dim3(NTHREADS), argv, lds, s));
    return KURA_OK;
}

// Split-group launches go through hipLaunchCooperativeKernel: its launch-time
// check (grid vs the occupancy query) turns a grid that cannot be co-resident
// into an error instead of barriers that time out (KURA_F_BARRIER).
// Diagnostic (KURA_XL_LAUNCH=plain in the environment at kura_create): a plain
// hipLaunchKernel of the same grid, co-residency checked once by the occupancy
// query in kura_create -- the same kernel on the stream's ordinary queue
// instead of the runtime's cooperative queue (DESIGN.md section 6: the
// exit-time fault of rocprofv3-traced split-group runs).
template <typename... A>
static int launch_xl(bool plain, const void* fn, dim3 grid, size_t lds, hipStream_t s, A... args) {
    void* argv[] = {(void*)&args...};
    if (plain) {
        HIP_TRY(hipLaunchKernel(fn, grid, dim3(NTHREADS), argv, lds, s));
        return KURA_OK;
    }
    hipError_t e = hipLaunchCooperativeKernel(fn, grid, dim3(NTHREADS), argv, (unsigned)lds, s);
    if (e == hipErrorCooperativeLaunchTooLarge)
        return set_err(KURA_E_UNSUPPORTED, "split-group grid of %u workgroups cannot be co-resident", grid.x);
    if (e != hipSuccess) return set_err(KURA_E_HIP, "hipLaunchCooperativeKernel: %s", hipGetErrorString(e));
    return KURA_OK;
}

// Re-form every env's R1/R3 spectral accumulators from its ring (after the
// ring or the twiddle tables were replaced from the host); synchronous.
static int spec_rebuild(KuraHandle* h) {
    if (h->cfg.reward_kind == KURA_R_TEMP_CONST || h->cfg.n_bins == 0 || !h->have_spectral) return KURA_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(kura_spec_init_kernel, dim3(h->B), dim3(64), 0, 0, h->p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return KURA_OK;
}

extern "C" {

const char* kura_last_error(void) { return g_err; }
int kura_abi_version(void) { return KURA_ABI_VERSION; }

int kura_create(const KuraConfig* cfg, int device, KuraHandle** out) {
    if (!out) return set_err(KURA_E_INVALID, "null out");
    *out = nullptr;
    int rc = validate(cfg);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    KuraHandle* h = new (std::nothrow) KuraHandle();
    if (!h) return set_err(KURA_E_NOMEM, "handle");
    h->cfg = *cfg;
    h->device = device;
    const int N = cfg->n_osc, B = cfg->n_envs, W = cfg->window;
    const int Bp = (B + E_WG - 1) / E_WG * E_WG;
    h->B = B;
    h->xl = N > XL_NL;
    const int part = cfg->part_osc > 0 ? cfg->part_osc : XL_NL;
    if (h->xl && !((part == 256 || part == 512 || part == 1024) && N % part == 0)) {
        delete h;
        return set_err(KURA_E_INVALID, "part_osc=%d: expected 256, 512 or 1024 dividing n_osc=%d", part, N);
    }
    h->tpw = h->xl ? part / 256 : N / 256;
    h->ngroups = Bp / E_WG;
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
            h->ncu = ncu;
    }
#ifdef KURA_DEBUG
    // test hook (debug build only): cap the co-resident grid of split-group
    // launches, which exercises the persistent pair loop with few envs
    if (const char* e = getenv("KURA_XL_MAX_GRID")) {
        const int g = atoi(e);
        if (g > 0 && g < h->ncu) h->ncu = g;
    }
#endif
    const int npart = h->xl ? N / part : 1;
    if (h->xl && h->ncu < npart) {
        const int ncu = h->ncu;
        delete h;
        return set_err(KURA_E_UNSUPPORTED, "n_osc=%d needs %d co-resident workgroups, device has %d CUs", N, npart,
                       ncu);
    }
    h->sp = kura_coupling_of(cfg) == KURA_COUPLING_BF16X3;
    rc = KURA_OK;
    h->alpha_cap = coupling_image_alloc(N, h->sp, h->tpw);
    rc = rc ? rc : dalloc(&h->alpha_sw, h->alpha_cap);
    rc = rc ? rc : dalloc(&h->omega, (size_t)Bp * N);
    rc = rc ? rc : dalloc(&h->kn_env, (size_t)Bp);
    rc = rc ? rc : dalloc(&h->g_stim, (size_t)Bp * cfg->n_elec * N);
    rc = rc ? rc : dalloc(&h->g_rec, (size_t)Bp * N);
    rc = rc ? rc : dalloc(&h->ctab, (size_t)std::max(cfg->n_bins, 1) * W);
    rc = rc ? rc : dalloc(&h->stab, (size_t)std::max(cfg->n_bins, 1) * W);
    rc = rc ? rc : dalloc(&h->y, (size_t)Bp * N);
    rc = rc ? rc : dalloc(&h->t, (size_t)Bp);
    rc = rc ? rc : dalloc(&h->step, (size_t)Bp);
    rc = rc ? rc : dalloc(&h->ring, (size_t)Bp * W);
    rc = rc ? rc : dalloc(&h->wpos, (size_t)Bp);
    rc = rc ? rc : dalloc(&h->R, (size_t)Bp * NSLOT * N);  // [Bp/16][NSLOT][N][16]
    rc = rc ? rc : dalloc(&h->pulse, (size_t)Bp * N);
    rc = rc ? rc : dalloc(&h->r2c, (size_t)W);
    rc = rc ? rc : dalloc(&h->spec, (size_t)Bp * 2 * std::max(cfg->n_bins, 1));
    rc = rc ? rc : dalloc(&h->stats, (size_t)KURA_NSTATS);
    rc = rc ? rc : dalloc(&h->stamps, (size_t)NWAVES * KURA_NSTAMP);
    rc = rc ? rc : dalloc(&h->eflags, (size_t)Bp);
    if (cfg->episode_cap > 0) {
        rc = rc ? rc : dalloc(&h->ep_lfp, (size_t)Bp * cfg->episode_cap);
        rc = rc ? rc : dalloc(&h->ep_len, (size_t)Bp);
    }
    if (h->xl) {
        rc = rc ? rc : dalloc(&h->xg, (size_t)h->ngroups * 2 * npart * xl_img(h->tpw));
        rc = rc ? rc : dalloc(&h->xred, (size_t)h->ngroups * 2 * npart * RC * E_WG);
        rc = rc ? rc : dalloc(&h->xredd, (size_t)h->ngroups * 2 * npart * RC * E_WG);
        rc = rc ? rc : dalloc(&h->gcnt, (size_t)h->ngroups * 16);
    }
    if (!rc) {  // every env starts with the config's gain float32(K/N)
        std::vector<float> kn((size_t)Bp, cfg->kn);
        if (hipMemcpy(h->kn_env, kn.data(), kn.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(KURA_E_HIP, "kn_env init");
    }
    if (!rc && cfg->padlen >= 1 && cfg->padlen < W) {  // R2: filtfilt(x)[-1] - mean = c . x
        std::vector<double> c((size_t)W);
        if (kura_r2_functional(cfg->bw_b, cfg->bw_a, cfg->bw_zi, W, cfg->padlen, c.data()) != 0)
            rc = set_err(KURA_E_NOMEM, "R2 functional");
        else if (hipMemcpy(h->r2c, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(KURA_E_HIP, "R2 functional upload");
    }
    if (!rc) rc = prepare_kernels(h->tpw, launch_lds(h), h->xl, h->sp);
    if (!rc && h->xl) {
        const char* e = getenv("KURA_XL_LAUNCH");
        h->xl_plain = e && !strcmp(e, "plain");
        if (h->xl_plain) {   // the cooperative launch's co-residency check, done once here
            const void *ks, *kr;
            select_kernels(h->tpw, h->xl, h->sp, &ks, &kr);
            for (const void* k : {ks, kr}) {
                int nb = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, NTHREADS, launch_lds(h)) != hipSuccess ||
                    nb < 1)
                    rc = set_err(KURA_E_UNSUPPORTED, "split-group kernel does not fit a CU (occupancy %d)", nb);
            }
        }
    }
    if (rc) {
        int keep = rc;
        kura_destroy(h);
        return keep;
    }
    fill_params(h);
    *out = h;
    return KURA_OK;
}

int kura_destroy(KuraHandle* h) {
    if (!h) return KURA_OK;
    (void)hipSetDevice(h->device);
    void* ptrs[] = {h->alpha_sw, h->alpha_dd, h->omega, h->kn_env, h->g_stim, h->g_rec, h->ctab, h->stab, h->y, h->t, h->step,
                    h->ring, h->wpos, h->R, h->pulse, h->r2c, h->spec, h->stats, h->stamps,
                    h->xg, h->xred, h->xredd, h->gcnt, h->ep_lfp, h->ep_len, h->met_scratch,
                    h->eflags};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    for (auto& kv : h->r2c_len) (void)hipFree(kv.second);
    delete h;
    return KURA_OK;
}

int kura_set_coupling(KuraHandle* h, const float* alpha) {
    if (!h || !alpha) return set_err(KURA_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    const int N = h->cfg.n_osc;
    // a failed upload leaves the handle without a coupling (and without a
    // dangling image pointer): set again only after every upload succeeded
    h->have_coupling = false;
    h->p.alpha_reuse = 0;
    const std::vector<float> sw = coupling_image(alpha, N, h->sp, h->tpw);
    if (sw.size() > h->alpha_cap) {   // the deduplicated image: sized to its distinct fragments
        HIP_TRY(hipDeviceSynchronize());   // no launch in flight reads the old image
        float* old = h->alpha_sw;
        h->alpha_sw = nullptr;
        h->alpha_cap = 0;
        h->p.alpha_sw = nullptr;
        HIP_TRY(hipFree(old));
        if (int rc = dalloc(&h->alpha_sw, sw.size())) return rc;
        h->alpha_cap = sw.size();
        h->p.alpha_sw = h->alpha_sw;
    }
    HIP_TRY(hipMemcpy(h->alpha_sw, sw.data(), sw.size() * sizeof(float), hipMemcpyHostToDevice));
    if (h->sp && !h->xl) {   // K1's BF16X3 reset reads alpha through the deduplicated image
        const std::vector<float> dd = split_alpha_dedup(alpha, N);
        if (dd.size() > h->alpha_dd_cap) {
            HIP_TRY(hipDeviceSynchronize());
            float* old = h->alpha_dd;
            h->alpha_dd = nullptr;
            h->alpha_dd_cap = 0;
            h->p.alpha_dd = nullptr;
            h->p.alpha_dd_bytes = 0;
            if (old) HIP_TRY(hipFree(old));
            if (int rc = dalloc(&h->alpha_dd, dd.size())) return rc;
            h->alpha_dd_cap = dd.size();
            h->p.alpha_dd = h->alpha_dd;
            h->p.alpha_dd_bytes = (unsigned)(dd.size() * sizeof(float));
        }
        HIP_TRY(hipMemcpy(h->alpha_dd, dd.data(), dd.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // K1's BF16X3 step GEMM at N = 1024: the shift-reuse form where the data allow it
    h->p.alpha_reuse = h->sp && !h->xl && alpha_reuse_allowed() &&
                       alpha_shift_reuse(reinterpret_cast<const uint16_t*>(sw.data()), N);
    h->have_coupling = true;
    return KURA_OK;
}

int kura_alpha_reuse(KuraHandle* h) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    return h->have_coupling && h->p.alpha_reuse ? 1 : 0;
}

int kura_alpha_reuse_detect(const float* alpha, int n_osc) {
    if (!alpha) return set_err(KURA_E_INVALID, "null argument");
    if (n_osc != 1024) return 0;
    std::vector<uint16_t> sp((size_t)n_osc * n_osc * 3);
    split_alpha(alpha, sp.data(), n_osc);
    return alpha_shift_reuse(sp.data(), n_osc) ? 1 : 0;
}

int kura_set_env_params(KuraHandle* h, int env0, int n, const float* omega, const double* g_stim,
                        const double* g_rec) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    if (env0 < 0 || n < 0 || env0 + n > h->B) return set_err(KURA_E_INVALID, "env range [%d,%d) outside [0,%d)", env0, env0 + n, h->B);
    HIP_TRY(hipSetDevice(h->device));
    const size_t N = h->cfg.n_osc;
    if (omega)
        HIP_TRY(hipMemcpy(h->omega + (size_t)env0 * N, omega, (size_t)n * N * sizeof(float), hipMemcpyHostToDevice));
    if (g_stim)
        HIP_TRY(hipMemcpy(h->g_stim + (size_t)env0 * h->cfg.n_elec * N, g_stim,
                          (size_t)n * h->cfg.n_elec * N * sizeof(double), hipMemcpyHostToDevice));
    if (g_rec && h->cfg.n_rec > 0) {
        // records = mean(cos(theta) * G) with G = g_0 + g_1 + ... in recorder
        // order (oracle lfp_row); identical to env.py:409-411 for one recorder
        std::vector<double> G((size_t)n * N);
        const int nr = h->cfg.n_rec;
        for (int b = 0; b < n; ++b)
            for (size_t i = 0; i < N; ++i) {
                double acc = g_rec[((size_t)b * nr) * N + i];
                for (int r = 1; r < nr; ++r) acc = acc + g_rec[((size_t)b * nr + r) * N + i];
                G[(size_t)b * N + i] = acc;
            }
        HIP_TRY(hipMemcpy(h->g_rec + (size_t)env0 * N, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (omega && g_stim) h->have_params = true;
    return KURA_OK;
}

int kura_set_env_gain(KuraHandle* h, int env0, int n, const float* kn) {
    if (!h || !kn) return set_err(KURA_E_INVALID, "null argument");
    if (env0 < 0 || n < 0 || env0 + n > h->B) return set_err(KURA_E_INVALID, "env range [%d,%d) outside [0,%d)", env0, env0 + n, h->B);
    for (int b = 0; b < n; ++b)
        if (!(kn[b] == kn[b])) return set_err(KURA_E_INVALID, "kn[%d] is nan", env0 + b);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy(h->kn_env + env0, kn, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return KURA_OK;
}

int kura_set_spectral(KuraHandle* h, const double* cos_tab, const double* sin_tab) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    const size_t n = (size_t)h->cfg.n_bins * h->cfg.window;
    if (n) {
        if (!cos_tab || !sin_tab) return set_err(KURA_E_INVALID, "null twiddle table");
        HIP_TRY(hipMemcpy(h->ctab, cos_tab, n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->stab, sin_tab, n * sizeof(double), hipMemcpyHostToDevice));
    }
    h->have_spectral = true;
    if (h->was_reset) return spec_rebuild(h);  // accumulators of the new tables
    return KURA_OK;
}

static int launch_common_checks(KuraHandle* h) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    if (!h->have_coupling) return set_err(KURA_E_STATE, "kura_set_coupling not called");
    if (!h->have_params) return set_err(KURA_E_STATE, "kura_set_env_params not called");
    if (!h->have_spectral && h->cfg.reward_kind != KURA_R_TEMP_CONST)
        return set_err(KURA_E_STATE, "kura_set_spectral not called");
    return KURA_OK;
}

// Grid of a step/reset launch.  N <= 1024: one workgroup per env group.
// Split groups: a persistent grid, a multiple of npart and at most one
// workgroup per CU, so all parts of a group are co-resident (their barriers
// spin on each other); the arrival counters are zeroed first.
static int launch_grid(KuraHandle* h, hipStream_t s, dim3* grid) {
    if (!h->xl) {
        *grid = dim3(h->ngroups);
        return KURA_OK;
    }
    const int npart = h->p.npart;
    int g = (h->ncu / npart) * npart;
    if (g > h->p.npairs) g = h->p.npairs;
    HIP_TRY(hipMemsetAsync(h->gcnt, 0, (size_t)h->ngroups * 16 * sizeof(unsigned), s));
    *grid = dim3(g);
    return KURA_OK;
}


int kura_reset(KuraHandle* h, const uint8_t* mask, const float* theta0, float* obs, void* stream) {
    int rc = launch_common_checks(h);
    if (rc) return rc;
    if (!theta0) return set_err(KURA_E_INVALID, "null theta0");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(h->stats, 0, 5 * sizeof(unsigned long long), s));  // per-call fields
    dim3 grid;
    rc = launch_grid(h, s, &grid);
    if (rc) return rc;
    const size_t lds = launch_lds(h);
    const void *ks, *kr;
    rc = select_kernels(h->tpw, h->xl, h->sp, &ks, &kr);
    if (rc) return rc;
    rc = h->xl ? launch_xl(h->xl_plain, kr, grid, lds, s, h->p, mask, theta0, obs)
               : launch_plain(kr, grid, lds, s, h->p, mask, theta0, obs);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    h->was_reset = true;
    return KURA_OK;
}

int kura_step(KuraHandle* h, const float* action, float* obs, double* reward, uint8_t* done, float* lfp_true,
              double* lfp_rec, int32_t* nsamp, void* stream) {
    int rc = launch_common_checks(h);
    if (rc) return rc;
    if (!h->was_reset) return set_err(KURA_E_STATE, "kura_step before kura_reset");
    if (!action) return set_err(KURA_E_INVALID, "null action");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(h->stats, 0, 5 * sizeof(unsigned long long), s));  // per-call fields
    dim3 grid;
    rc = launch_grid(h, s, &grid);
    if (rc) return rc;
    const size_t lds = launch_lds(h);
    const void *ks, *kr;
    rc = select_kernels(h->tpw, h->xl, h->sp, &ks, &kr);
    if (rc) return rc;
    rc = h->xl ? launch_xl(h->xl_plain, ks, grid, lds, s, h->p, action, obs, reward, done, lfp_true, lfp_rec, nsamp)
               : launch_plain(ks, grid, lds, s, h->p, action, obs, reward, done, lfp_true, lfp_rec, nsamp);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return KURA_OK;
}

int kura_reward(KuraHandle* h, int kind, const double* window, const float* u0, double* reward, int n,
                void* stream) {
    if (!h || !window || !u0 || !reward) return set_err(KURA_E_INVALID, "null argument");
    if (n < 0 || n > h->B) return set_err(KURA_E_INVALID, "n=%d outside [0,%d]", n, h->B);
    if (kind == 0) kind = h->cfg.reward_kind;
    if (kind < 1 || kind > 3) return set_err(KURA_E_INVALID, "Wrong reward function! (%d)", kind);
    if (!h->have_spectral && kind != KURA_R_TEMP_CONST) return set_err(KURA_E_STATE, "kura_set_spectral not called");
    if (kind == KURA_R_TEMP_CONST && (h->cfg.padlen < 1 || h->cfg.padlen >= h->cfg.window))
        return set_err(KURA_E_INVALID, "padlen=%d", h->cfg.padlen);
    if (n == 0) return KURA_OK;
    HIP_TRY(hipSetDevice(h->device));
    DevParams p = h->p;
    p.reward_kind = kind;
    hipLaunchKernelGGL(kura_reward_kernel<WPL_MAX>, dim3(n), dim3(64), 0, (hipStream_t)stream, p, window, u0,
                       reward, n);
    HIP_TRY(hipGetLastError());
    return KURA_OK;
}

int kura_reward_n(KuraHandle* h, int kind, const double* x, int64_t len, int64_t ld, int n, const double* cos_tab,
                  const double* sin_tab, int n_bins, const double* u0, double* reward, void* stream) {
    if (!h || !x || !u0 || !reward) return set_err(KURA_E_INVALID, "null argument");
    if (n < 0) return set_err(KURA_E_INVALID, "n=%d", n);
    if (kind == 0) kind = h->cfg.reward_kind;
    if (kind < 1 || kind > 3) return set_err(KURA_E_INVALID, "Wrong reward function! (%d)", kind);
    if (len < 1 || len > (1 << 28) || ld < len) return set_err(KURA_E_INVALID, "len=%lld ld=%lld", (long long)len,
                                                               (long long)ld);
    if (kind != KURA_R_TEMP_CONST && (n_bins < 0 || (n_bins > 0 && (!cos_tab || !sin_tab))))
        return set_err(KURA_E_INVALID, "n_bins=%d needs both twiddle tables", n_bins);
    const int padlen = h->cfg.padlen;
    if (kind == KURA_R_TEMP_CONST && len <= padlen)  // scipy.signal.filtfilt's own check
        return set_err(KURA_E_INVALID, "The length of the input vector x must be greater than padlen, which is %d.",
                       padlen);
    if (n == 0) return KURA_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    DevParams p = h->p;
    p.reward_kind = kind;
    p.W = (int)len;
    const double* c = nullptr;
    if (kind == KURA_R_TEMP_CONST) {
        // the length-len functional, built once per length and kept with the
        // handle in a most-recently-used list of at most R2C_CACHE lengths
        for (size_t i = 0; i < h->r2c_len.size() && !c; ++i)
            if (h->r2c_len[i].first == (long long)len) {
                c = h->r2c_len[i].second;
                std::rotate(h->r2c_len.begin(), h->r2c_len.begin() + i, h->r2c_len.begin() + i + 1);
            }
        if (!c) {
            std::vector<double> hc((size_t)len);
            if (kura_r2_functional(h->cfg.bw_b, h->cfg.bw_a, h->cfg.bw_zi, (int)len, padlen, hc.data()) != 0)
                return set_err(KURA_E_NOMEM, "R2 functional of length %lld", (long long)len);
            if (h->r2c_len.size() >= R2C_CACHE) {   // evict the least recently used length: a queued
                HIP_TRY(hipDeviceSynchronize());     // launch may still read it
                HIP_TRY(hipFree(h->r2c_len.back().second));
                h->r2c_len.pop_back();
            }
            double* dc = nullptr;
            int rc = dalloc(&dc, (size_t)len);
            if (rc) return rc;
            HIP_TRY(hipMemcpy(dc, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice));
            h->r2c_len.insert(h->r2c_len.begin(), std::make_pair((long long)len, dc));
            c = dc;
        }
    }
    hipLaunchKernelGGL(kura_reward_n_kernel, dim3(n), dim3(64), 0, s, p, x, (long long)ld, cos_tab, sin_tab,
                       kind == KURA_R_TEMP_CONST ? 0 : n_bins, u0, reward, c, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(KURA_E_HIP, "kura_reward_n: %s", hipGetErrorString(e));
    return KURA_OK;
}

#ifdef KURA_DEBUG
// diagnostic (libkura_debug.so only, tools/coupling_dump_probe.py): keep the
// operand image and coupling sums of the first n sweeps of workgroup 0
// (N <= 1024) in dev_buf ([n][2][32][N] float32, device; NULL stops)
int kura_debug_gemm_dump(KuraHandle* h, float* dev_buf, int n) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    h->p.gemm_dump = dev_buf;
    h->p.gemm_dump_n = dev_buf ? n : 0;
    return KURA_OK;
}

// diagnostic (libkura_debug.so only, tools/record_probe.py)
int kura_debug_read_workspace(KuraHandle* h, float* out, int64_t n) {
    if (!h || !out) return set_err(KURA_E_INVALID, "null argument");
    const int64_t Bp = (int64_t)h->ngroups * E_WG;
    const int64_t total = Bp * NSLOT * (int64_t)h->cfg.n_osc;
    if (n < total) return set_err(KURA_E_INVALID, "n=%lld < workspace floats %lld", (long long)n, (long long)total);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->R, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
    return KURA_OK;
}
#endif

int kura_get_state(KuraHandle* h, float* y, double* t, int32_t* step, double* ring, int32_t* wpos) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t B = h->B, N = h->cfg.n_osc, W = h->cfg.window;
    if (y) HIP_TRY(hipMemcpy(y, h->y, B * N * sizeof(float), hipMemcpyDeviceToHost));
    if (t) HIP_TRY(hipMemcpy(t, h->t, B * sizeof(double), hipMemcpyDeviceToHost));
    if (step) HIP_TRY(hipMemcpy(step, h->step, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (ring) HIP_TRY(hipMemcpy(ring, h->ring, B * W * sizeof(double), hipMemcpyDeviceToHost));
    if (wpos) HIP_TRY(hipMemcpy(wpos, h->wpos, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    return KURA_OK;
}

int kura_set_state(KuraHandle* h, const float* y, const double* t, const int32_t* step, const double* ring,
                   const int32_t* wpos) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t B = h->B, N = h->cfg.n_osc, W = h->cfg.window;
    if (y) HIP_TRY(hipMemcpy(h->y, y, B * N * sizeof(float), hipMemcpyHostToDevice));
    if (t) HIP_TRY(hipMemcpy(h->t, t, B * sizeof(double), hipMemcpyHostToDevice));
    if (step) HIP_TRY(hipMemcpy(h->step, step, B * sizeof(int32_t), hipMemcpyHostToDevice));
    if (ring) HIP_TRY(hipMemcpy(h->ring, ring, B * W * sizeof(double), hipMemcpyHostToDevice));
    if (wpos) HIP_TRY(hipMemcpy(h->wpos, wpos, B * sizeof(int32_t), hipMemcpyHostToDevice));
    if (y && t && step && ring && wpos) h->was_reset = true;
    if (ring) return spec_rebuild(h);  // kura_set_spec restores the exact accumulators of a checkpoint
    return KURA_OK;
}

int kura_get_spec(KuraHandle* h, double* out) {
    if (!h || !out) return set_err(KURA_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = (size_t)h->B * 2 * h->cfg.n_bins;
    if (n) HIP_TRY(hipMemcpy(out, h->spec, n * sizeof(double), hipMemcpyDeviceToHost));
    return KURA_OK;
}

int kura_set_spec(KuraHandle* h, const double* in) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    if (!in) return spec_rebuild(h);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = (size_t)h->B * 2 * h->cfg.n_bins;
    if (n) HIP_TRY(hipMemcpy(h->spec, in, n * sizeof(double), hipMemcpyHostToDevice));
    return KURA_OK;
}

// ---- episode metrics: calc_psd_for_simple_eval (evaluate_HF_DBS.py:122-135)
// and the callback's envelope statistics (custom_callbacks.py:146-148), both
// on Bluestein DFTs (kura_fft.inc).  The signals of one call are processed in
// chunks that share one scratch buffer per handle: metric calls on a handle
// must be issued on one stream (kura.h).  Growing the buffer first waits for
// the device explicitly (work queued on any stream may still use the old
// buffer), then releases it.
static long long conv_len(long long ld) {  // power of two >= 2*ld - 1
    long long M = 1;
    while (M < 2 * ld - 1) M <<= 1;
    return M < 4 ? 4 : M;
}

static int met_scratch(KuraHandle* h, size_t bytes) {
    if (bytes <= h->met_scratch_n) return KURA_OK;
    if (h->met_scratch) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipFree(h->met_scratch));
    }
    h->met_scratch = nullptr;
    h->met_scratch_n = 0;
    HIP_TRY(hipMalloc(&h->met_scratch, bytes));
    h->met_scratch_n = bytes;
    return KURA_OK;
}

// signals per chunk: the FFT buffers (4 * M complex per signal) within ~2 GiB
static int met_chunk(long long M, int n) {
    const long long per = 64LL * M;
    long long c = (2LL << 30) / per;
    c = c < 1 ? 1 : (c > 256 ? 256 : c);
    return (int)(c < n ? c : (n > 0 ? n : 1));
}

static unsigned met_grid(long long M) {
    const long long g = (M + FFT_THREADS - 1) / FFT_THREADS;
    return (unsigned)(g > 1024 ? 1024 : g);
}

// Bluestein forward DFT of the prepared chunk (buf: A even / B odd slots):
// returns the buffer whose even slots hold c = M * (a conv b) and sets *bloc
// to the one whose odd slots hold FFT(b).
static double2* blu_forward(double2* buf, double2* tmp, long long M, int cnt, hipStream_t st, double2** bloc) {
    double2* r1 = fft_pow2(buf, tmp, (int)M, 2 * cnt, M, -1.0, st);
    double2* fr = r1 == buf ? tmp : buf;
    hipLaunchKernelGGL(kura_blu_mul, dim3(met_grid(M), cnt), dim3(FFT_THREADS), 0, st, r1, (const double2*)r1,
                       (int)M);
    *bloc = r1;
    return fft_pow2(r1, fr, (int)M, cnt, 2 * M, 1.0, st);
}

// filter groups: the Butterworth filtfilt runs one lane per signal and is
// serial in time, so every signal of a group is filtered in one launch (its
// latency is paid once per group, not once per FFT chunk)
#define PSD_FGROUP 2048

static int psd_launch(KuraHandle* h, const float* sig, const int32_t* len, int64_t ld, int n, int episode,
                      const uint8_t* mask, double psd_dt, double beta_a, double beta_b, double* out, void* stream) {
    if (!(psd_dt > 0.0) || !(beta_b > beta_a)) return set_err(KURA_E_INVALID, "psd_dt/beta band");
    if (h->cfg.padlen < 1) return set_err(KURA_E_INVALID, "padlen=%d", h->cfg.padlen);
    HIP_TRY(hipSetDevice(h->device));
    const long long M = conv_len(ld);
    const int cnt = met_chunk(M, n);
    const long long xld = ld, tld = ld + 2 * (long long)h->cfg.padlen, yld = ld / 2 + 1 + 72;
    // filter group: up to PSD_FGROUP signals, sized like met_chunk from a ~2 GiB
    // budget for its 8 * (xld + tld) bytes per signal (long signals: smaller groups)
    long long fgb = (2LL << 30) / (8LL * (xld + tld));
    fgb = fgb < 1 ? 1 : (fgb > PSD_FGROUP ? PSD_FGROUP : fgb);
    const int fg = n < fgb ? (n > 0 ? n : 1) : (int)fgb;
    int rc = met_scratch(h, (size_t)cnt * (64 * M + 8 * yld) + (size_t)fg * 8 * (xld + tld));
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)stream;
    double2* buf = (double2*)h->met_scratch;
    double2* tmp = buf + (size_t)2 * cnt * M;
    double* y1 = (double*)(tmp + (size_t)2 * cnt * M);
    double* xd = y1 + (size_t)cnt * yld;
    double* ftmp = xd + (size_t)fg * xld;
    for (int g0 = 0; g0 < n; g0 += fg) {
        const int gc = n - g0 < fg ? n - g0 : fg;
        hipLaunchKernelGGL(kura_psd_filt, dim3((gc + 63) / 64), dim3(64), 0, st, h->p, sig, len, (long long)ld, g0,
                           gc, episode, mask, xd, xld, ftmp, tld);
        for (int j0 = g0; j0 < g0 + gc; j0 += cnt) {
            const int c = g0 + gc - j0 < cnt ? g0 + gc - j0 : cnt;
            hipLaunchKernelGGL(kura_blu_prep, dim3(met_grid(M), c), dim3(FFT_THREADS), 0, st, h->p, sig, len,
                               (long long)ld, j0, episode, mask, (const double*)(xd + (size_t)(j0 - g0) * xld), xld,
                               (int)M, buf);
            double2* bloc;
            double2* r = blu_forward(buf, tmp, M, c, st, &bloc);
            hipLaunchKernelGGL(kura_psd_band, dim3(c), dim3(FFT_THREADS), 0, st, h->p, sig, len, (long long)ld, j0,
                               episode, mask, (int)M, (const double2*)r, y1, yld, psd_dt, beta_a, beta_b, out);
            HIP_TRY(hipGetLastError());
        }
    }
    return KURA_OK;
}

int kura_psd_bbpow(KuraHandle* h, const float* sig, const int32_t* len, int64_t ld, int n, double psd_dt,
                   double beta_a, double beta_b, double* out, void* stream) {
    if (!h || !sig || !len || !out || n < 0 || ld < 2 || ld > (1 << 24)) return set_err(KURA_E_INVALID, "bad argument");
    return psd_launch(h, sig, len, ld, n, 0, nullptr, psd_dt, beta_a, beta_b, out, stream);
}

int kura_episode_bbpow(KuraHandle* h, const uint8_t* mask, double psd_dt, double beta_a, double beta_b,
                       double* out, void* stream) {
    if (!h || !out) return set_err(KURA_E_INVALID, "null argument");
    if (!h->ep_lfp) return set_err(KURA_E_STATE, "episode record disabled (KuraConfig.episode_cap == 0)");
    return psd_launch(h, nullptr, nullptr, h->cfg.episode_cap, h->B, 1, mask, psd_dt, beta_a, beta_b, out,
                      stream);
}

static int env_launch(KuraHandle* h, const float* sig, const int32_t* len, int64_t ld, int n, int episode,
                      const uint8_t* mask, double* out, void* stream) {
    HIP_TRY(hipSetDevice(h->device));
    const long long M = conv_len(ld);
    const int cnt = met_chunk(M, n);
    int rc = met_scratch(h, (size_t)cnt * 64 * M);
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)stream;
    double2* buf = (double2*)h->met_scratch;
    double2* tmp = buf + (size_t)2 * cnt * M;
    const unsigned g = met_grid(M);
    for (int j0 = 0; j0 < n; j0 += cnt) {
        const int c = n - j0 < cnt ? n - j0 : cnt;
        hipLaunchKernelGGL(kura_blu_prep, dim3(g, c), dim3(FFT_THREADS), 0, st, h->p, sig, len, (long long)ld, j0,
                           episode, mask, (const double*)nullptr, 0LL, (int)M, buf);
        double2* bloc;
        double2* r2 = blu_forward(buf, tmp, M, c, st, &bloc);   // even slots: M * DFT_L(x) / w
        hipLaunchKernelGGL(kura_env_mid, dim3(g, c), dim3(FFT_THREADS), 0, st, h->p, sig, len, (long long)ld, j0,
                           episode, mask, (int)M, r2);
        double2* fr = r2 == buf ? tmp : buf;
        double2* r3 = fft_pow2(r2, fr, (int)M, c, 2 * M, -1.0, st);
        hipLaunchKernelGGL(kura_blu_mul, dim3(g, c), dim3(FFT_THREADS), 0, st, r3, (const double2*)bloc, (int)M);
        double2* r4 = fft_pow2(r3, r3 == buf ? tmp : buf, (int)M, c, 2 * M, 1.0, st);
        hipLaunchKernelGGL(kura_env_stats, dim3(c), dim3(FFT_THREADS), 0, st, h->p, sig, len, (long long)ld, j0,
                           episode, mask, (int)M, (const double2*)r4, out);
        HIP_TRY(hipGetLastError());
    }
    return KURA_OK;
}

int kura_envelope_stats(KuraHandle* h, const float* sig, const int32_t* len, int64_t ld, int n, double* out,
                        void* stream) {
    if (!h || !sig || !len || !out || n < 0 || ld < 1 || ld > (1 << 24)) return set_err(KURA_E_INVALID, "bad argument");
    return env_launch(h, sig, len, ld, n, 0, nullptr, out, stream);
}

int kura_episode_envelope_stats(KuraHandle* h, const uint8_t* mask, double* out, void* stream) {
    if (!h || !out) return set_err(KURA_E_INVALID, "null argument");
    if (!h->ep_lfp) return set_err(KURA_E_STATE, "episode record disabled (KuraConfig.episode_cap == 0)");
    return env_launch(h, nullptr, nullptr, h->cfg.episode_cap, h->B, 1, mask, out, stream);
}

int kura_set_row_capture(KuraHandle* h, float* rows_dev) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    h->p.rows = rows_dev;
    return KURA_OK;
}

int kura_set_transient_capture(KuraHandle* h, double* lfp_dev) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    h->p.lfp_tr = lfp_dev;
    return KURA_OK;
}

int kura_set_transient_rows(KuraHandle* h, float* rows_dev) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    // the save passes address one env group's rows with 32-bit byte offsets
    if (rows_dev && (double)16 * h->p.n_tr * h->cfg.n_osc * 4 > 2147483647.0 - 64)
        return set_err(KURA_E_INVALID, "transient rows of 16 envs (%d x %d floats each) exceed 2 GiB", h->p.n_tr,
                       h->cfg.n_osc);
    h->p.rows_tr = rows_dev;
    return KURA_OK;
}

int kura_transient_len(KuraHandle* h) {
    if (!h) return set_err(KURA_E_INVALID, "null handle");
    return h->p.n_tr;
}

int kura_get_env_flags(KuraHandle* h, int32_t* out_dev, void* stream) {
    if (!h || !out_dev) return set_err(KURA_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(out_dev, h->eflags, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return KURA_OK;
}

int kura_get_stats(KuraHandle* h, int64_t* out, int n) {
    if (!h || !out || n < 0) return set_err(KURA_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v[KURA_NSTATS];
    HIP_TRY(hipMemcpy(v, h->stats, sizeof(v), hipMemcpyDeviceToHost));
    for (int i = 0; i < n && i < KURA_NSTATS; ++i) out[i] = (int64_t)v[i];
    return KURA_OK;
}

// Phase cycle counters of KURA_STAMPS builds (zeros otherwise): [NWAVES][8],
// summed over workgroups since the last read; reading clears them.
int kura_get_stamps(KuraHandle* h, uint64_t* out /* NWAVES*KURA_NSTAMP */) {
    if (!h || !out) return set_err(KURA_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->stamps, NWAVES * KURA_NSTAMP * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(h->stamps, 0, NWAVES * KURA_NSTAMP * sizeof(uint64_t)));
    return KURA_OK;
}

// ---- diagnostics used by the GPU parity tests (not on the step path) ------
int kura_selftest_math(const float* x, const float* y, float* out, int n) {
    if (n <= 0 || !x || !y || !out) return set_err(KURA_E_INVALID, "bad args");
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    int rc = dalloc(&dx, n);
    rc = rc ? rc : dalloc(&dy, n);
    rc = rc ? rc : dalloc(&dout, (size_t)n * KURA_SELFTEST_MATH_W);
    if (!rc) {
        (void)hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice);
        (void)hipMemcpy(dy, y, n * sizeof(float), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(kura_selftest_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, dout, n);
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = set_err(KURA_E_HIP, "selftest_math: %s", hipGetErrorString(e));
        else (void)hipMemcpy(out, dout, (size_t)n * KURA_SELFTEST_MATH_W * sizeof(float), hipMemcpyDeviceToHost);
    }
    (void)hipFree(dx);
    (void)hipFree(dy);
    (void)hipFree(dout);
    return rc;
}

static int g_selftest_reuse = 0;   // GEMM form of the last kura_selftest_coupling
int kura_selftest_alpha_reuse(void) { return g_selftest_reuse; }

int kura_selftest_coupling(const float* X /* 32*N */, const float* alpha /* N*N */, float* Y /* 32*N */, int N,
                           int coupling) {
    if (N != 256 && N != 512 && N != 1024) return set_err(KURA_E_UNSUPPORTED, "N=%d", N);
    if (coupling != KURA_COUPLING_AUTO && coupling != KURA_COUPLING_F32 && coupling != KURA_COUPLING_BF16X3)
        return set_err(KURA_E_INVALID, "coupling=%d", coupling);
    const bool sp = coupling != KURA_COUPLING_F32;   // AUTO = BF16X3 (at every N, kura_coupling_of)
    const std::vector<float> sw = coupling_image(alpha, N, sp, N / 256);
    // the production dispatch (kura_set_coupling): the shift-reuse form where the data allow it
    int reuse = sp && alpha_reuse_allowed() && alpha_shift_reuse(reinterpret_cast<const uint16_t*>(sw.data()), N);
    g_selftest_reuse = reuse;
    float *dX = nullptr, *dA = nullptr, *dY = nullptr;
    int rc = dalloc(&dX, (size_t)32 * N);
    rc = rc ? rc : dalloc(&dA, sw.size());
    rc = rc ? rc : dalloc(&dY, (size_t)32 * N);
    const size_t lds = (size_t)xs_floats(N) * sizeof(float);
    const void* k = selftest_gemm_kernel(N / 256, sp);
    if (!rc && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        rc = set_err(KURA_E_HIP, "selftest_gemm: LDS attribute");
    if (!rc) {
        (void)hipMemcpy(dX, X, (size_t)32 * N * sizeof(float), hipMemcpyHostToDevice);
        (void)hipMemcpy(dA, sw.data(), sw.size() * sizeof(float), hipMemcpyHostToDevice);
        void* argv[] = {(void*)&dX, (void*)&dA, (void*)&dY, (void*)&N, (void*)&reuse};
        hipError_t e = hipLaunchKernel(k, dim3(1), dim3(NTHREADS), argv, lds, 0);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = set_err(KURA_E_HIP, "selftest_gemm: %s", hipGetErrorString(e));
        else (void)hipMemcpy(Y, dY, (size_t)32 * N * sizeof(float), hipMemcpyDeviceToHost);
    }
    (void)hipFree(dX);
    (void)hipFree(dA);
    (void)hipFree(dY);
    return rc;
}

int kura_selftest_gemm(const float* X, const float* alpha, float* Y, int N) {
    return kura_selftest_coupling(X, alpha, Y, N, KURA_COUPLING_F32);
}

}  // extern "C"
