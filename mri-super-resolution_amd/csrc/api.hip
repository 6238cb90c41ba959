// The library's own state (error string, profiler, launch counters, and the table of diagnostic switches, which has to see every
// unit's) and the SIREN network path: the fused fit / forward / reconstruct orchestration and the layer-wise backward entry points
// that share its helpers.  Every other family's entry points are at the end of the unit that owns its kernels.  Nothing here
// allocates device memory or synchronises (except inr_prof_read and inr_device_caps, which are not on the hot path).
#include <math.h>
#include <stdarg.h>

#include <mutex>
#include <vector>

#include "internal.h"

namespace inr {

// ---- error string -------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- profiler -------------------------------------------------------------------------------------
struct ProfState {
    std::mutex mu;
    bool enabled = false;
    std::vector<hipEvent_t> pool;                    // recycled events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[KC_COUNT];
    hipEvent_t open[KC_COUNT] = {nullptr, nullptr, nullptr, nullptr};
    int depth[KC_COUNT] = {0, 0, 0, 0};
    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
static ProfState g_prof;
bool prof_enabled() { return g_prof.enabled; }

// ---- launch-family counters (inr_launch_count) ------------------------------------------------------------------------
// one table for every family (common.h: LaunchFamily and the bases beside it)
static std::atomic<long long> g_launches[LF_TABLE];
void count_launch(int family) {
    if (family >= 0 && family < LF_TABLE) g_launches[family].fetch_add(1, std::memory_order_relaxed);
}
// scopes of one class may nest (a launcher calling another launcher): only the outermost pair is recorded
void prof_begin(int kc, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (g_prof.depth[kc]++ > 0) return;
    hipEvent_t e = g_prof.get();
    (void)hipEventRecord(e, s);
    g_prof.open[kc] = e;
}
void prof_end(int kc, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (--g_prof.depth[kc] > 0) return;
    hipEvent_t e = g_prof.get();
    (void)hipEventRecord(e, s);
    g_prof.spans[kc].push_back({g_prof.open[kc], e});
    g_prof.open[kc] = nullptr;
}

// ---- switches only this file reads (the others: internal.h) ------------------------------------------------------------------------
static tune_int g_small_multi{1};  // key 12, small networks: 1 = persistent multi-step kernel (default), 0 = two launches per step
static tune_int g_h3_serpentine{1};   // key 5
static tune_int g_hp{1};  // key 7: pre-split (HL32) GEMM path inside the fused entry points; inr_debug_set(7, 0) falls back to gemm_h3

// ---- shared helpers ---------------------------------------------------------------------------------
static int check_desc(const inr_siren_desc_t* d) {
    INR_REQUIRE(d != nullptr, INR_E_INVALID, "siren descriptor is null");
    INR_REQUIRE(d->in_features >= 1 && d->hidden_features >= 1 && d->hidden_layers >= 0 && d->out_features >= 1,
                INR_E_INVALID, "bad siren descriptor (in=%d hidden=%d layers=%d out=%d)", d->in_features,
                d->hidden_features, d->hidden_layers, d->out_features);
    return 0;
}

Layout make_layout(const inr_siren_desc_t* d) {
    Layout L;
    L.n_sine = 1 + d->hidden_layers;
    long long off = 0;
    for (int l = 0; l <= L.n_sine; ++l) {
        const int fin = (l == 0) ? d->in_features : d->hidden_features;
        const int fout = (l == L.n_sine) ? d->out_features : d->hidden_features;
        L.fan_in.push_back(fin);
        L.fan_out.push_back(fout);
        L.w_off.push_back(off);
        off += (long long)round_up((size_t)fin * fout, 4);
        L.b_off.push_back(off);
        off += (long long)round_up((size_t)fout, 4);
    }
    L.total = off;
    return L;
}

static size_t max2(size_t a, size_t b) { return a > b ? a : b; }

static size_t param_grad_ws_floats(int64_t n, int in_f, int out_f) {
    const int s1 = param_grad_splits(n, in_f, out_f), s2 = hp_param_grad_splits(n, in_f, out_f);
    const int splits = s1 > s2 ? s1 : s2;
    const size_t len = (size_t)in_f * out_f;
    const size_t slabs = (size_t)splits * len + (size_t)reduce_tmp_floats(splits, (int64_t)len);
    return max2(slabs, (size_t)colsum_ws_floats(n, out_f, 1));
}

// gW = dz^T x (row-split slabs + fixed-order reduce); gb = colsum(dz) when requested
static int param_grad(float* gW, float* gb, const float* dz, const float* x, int64_t n, int in_f, int out_f,
                      float* ws, hipStream_t st, const H3Args* h3 = nullptr) {
    const int splits = param_grad_splits(n, in_f, out_f);
    const int64_t len = (int64_t)in_f * out_f;
    if (int rc = gemm_param_grad_slabs(ws, splits, dz, x, n, in_f, out_f, st, h3)) return rc;
    if (int rc = launch_reduce_slabs(gW, ws, splits, len, ws + (int64_t)splits * len, st)) return rc;
    if (gb) {
        if (int rc = launch_colsum(gb, dz, nullptr, n, out_f, 1, ws, st)) return rc;
    }
    return 0;
}

static size_t input_grad_ws_floats(int64_t n, int in_f) {
    const int64_t rows = input_grad_colsum_rows(n);
    return max2((size_t)(rows * in_f + reduce_tmp_floats(rows, in_f)), (size_t)colsum_ws_floats(n, in_f, 1));
}

// dz_prev = (dz W) * dact_prev; gb_prev (nullable) = colsum(dz_prev), fused into the GEMM epilogue when the
// fast kernel runs, otherwise a separate column-sum pass
static int input_grad(float* dz_prev, float* gb_prev, const float* dz, const float* W, const float* dact_prev,
                      int64_t n, int in_f, int out_f, float* ws, hipStream_t st, const H3Args* h3 = nullptr) {
    int slab_rows = 0;
    float* slab = (gb_prev && dact_prev) ? ws : nullptr;
    if (int rc = gemm_input_grad(dz_prev, dz, W, dact_prev, n, in_f, out_f, slab, &slab_rows, st, h3)) return rc;
    if (!gb_prev) return 0;
    if (slab_rows > 0) return launch_reduce_slabs(gb_prev, ws, slab_rows, in_f, ws + (int64_t)slab_rows * in_f, st);
    return launch_colsum(gb_prev, dz_prev, nullptr, n, in_f, 1, ws, st);
}

// ---- split-GEMM context of one network in one workspace ------------------------------------------------------------------------
// A region of the caller's workspace: the scale slots (common.h: HpSlots), the scratch of the per-step weight statistics, then 8
// bytes per weight, layer after layer.  The split-fp16 path (gemm_h3.inc) keeps four fp16 planes per layer there (hi, lo, hiT,
// loT), the pre-split path (gemm_hp.inc) two HL32 images ([out][in], then [in][out]).
struct SplitCtx {
    bool on = false;                    // false: the network takes the fp32 kernels, nothing below is set
    HpSlots slots;
    unsigned* part = nullptr;           // scratch of the per-step weight statistics (gemm_hp.inc)
    char* planes = nullptr;
    long long w_first[HpSlots::MAX_LAYERS], w_count[HpSlots::MAX_LAYERS];   // weights before sine layer l / of sine layer l

    // gemm_h3.inc: fp16 planes
    const _Float16* h3_planes(int l) const { return reinterpret_cast<const _Float16*>(planes) + 4 * w_first[l]; }
    // gemm_hp.inc: HL32 images and the scales of the operands
    char* w_hl(int l) const { return planes + 8 * w_first[l]; }
    char* wT_hl(int l) const { return w_hl(l) + 4 * w_count[l]; }
    HpScale w_scale(int l) const { HpScale s; s.meas = slots.w_max(l); s.mul = 1.f; return s; }
    HpScale x_scale() const { HpScale s; s.meas = slots.x_max(); s.mul = 1.f; return s; }
    // input of sine layer l: the network input (measured max|x|) or the output of layer l - 1, whose image is scaled from the
    // a-priori bound of that layer (written by the per-step weight preparation: gemm_hp.inc, act_bound)
    HpScale act_scale(int l) const {
        if (l == 0) return x_scale();
        HpScale s;
        s.wn = slots.act_bound(l - 1);
        s.mul = 1.f;
        s.kmax = 40;
        return s;
    }
};
static bool h3_eligible(const Layout& L) {
    if (!g_h3 || L.n_sine > HpSlots::MAX_LAYERS) return false;
    for (int l = 0; l < L.n_sine; ++l)
        if (L.fan_in[l] % 32 != 0 || L.fan_out[l] % 32 != 0) return false;
    return true;
}
static bool hp_eligible(const inr_siren_desc_t* d, const Layout& L) {
    if (!g_hp || !g_h3 || g_force_generic || !h3_eligible(L)) return false;
    return d->out_features == 1 && hp_head_ok(d->hidden_features);
}
static size_t split_ctx_bytes(const Layout& L) {      // (reserved whether or not the network is eligible)
    long long w = 0;
    for (int l = 0; l < L.n_sine; ++l) w += (long long)L.fan_in[l] * L.fan_out[l];
    return round_up(HpSlots::BYTES + hp_prep_part_bytes() + h3_planes_bytes(w), 256);
}
// the context inside `region` (split_ctx_bytes(L) bytes) when the network is eligible, else one that is off
static SplitCtx split_ctx(const Layout& L, char* region) {
    SplitCtx c;
    if (!h3_eligible(L)) return c;
    c.on = true;
    c.slots.base = reinterpret_cast<unsigned*>(region);
    c.part = reinterpret_cast<unsigned*>(region + HpSlots::BYTES);
    c.planes = region + HpSlots::BYTES + hp_prep_part_bytes();
    long long first = 0;
    for (int l = 0; l < L.n_sine; ++l) {
        c.w_first[l] = first;
        c.w_count[l] = (long long)L.fan_in[l] * L.fan_out[l];
        first += c.w_count[l];
    }
    return c;
}
// split every sine layer's weights (once per optimizer step / forward call) and zero the dz slots
static int h3_refresh_weights(const SplitCtx& c, const Layout& L, const float* params, hipStream_t st) {
    const float* W[HpSlots::MAX_LAYERS];
    for (int l = 0; l < L.n_sine; ++l) W[l] = params + L.w_off[l];
    return h3_weight_split(W, L.fan_out.data(), L.fan_in.data(), L.n_sine, reinterpret_cast<_Float16*>(c.planes), c.slots.w_max(0),
                           c.slots.w_max(0), 2 * HpSlots::MAX_LAYERS, st);   // (w_max and dz_max are adjacent: both zeroed)
}
static H3Args h3_forward_args(const SplitCtx& c, int l) {
    H3Args a;
    a.a_amax = (l == 0) ? c.slots.x_max() : nullptr;   // sine outputs are in [-1, 1]; the network input is whatever it is
    a.b_amax = c.slots.w_max(l);
    a.Bh = c.h3_planes(l);
    a.Bl = a.Bh + c.w_count[l];
    a.reverse_m = g_h3_serpentine ? (l & 1) : 0;      // layer l+1 starts where layer l stopped writing
    return a;
}
static H3Args h3_input_grad_args(const SplitCtx& c, int l) {
    H3Args a;
    a.a_amax = c.slots.dz_max(l);
    a.b_amax = c.slots.w_max(l);
    a.Bh = c.h3_planes(l) + 2 * c.w_count[l];
    a.Bl = a.Bh + c.w_count[l];
    a.amax_out = c.slots.dz_max(l - 1);
    // backward chain: head pass (front to back) -> dW_L (back to front) -> dX_L (front to back) -> dW_{L-1} ... : every
    // kernel starts on the rows the one before it touched last
    a.reverse_m = 0;
    return a;
}
static H3Args h3_param_grad_args(const SplitCtx& c, int l) {
    H3Args a;
    a.a_amax = c.slots.dz_max(l);
    a.b_amax = (l == 0) ? c.slots.x_max() : nullptr;
    a.reverse_m = g_h3_serpentine ? 1 : 0;
    return a;
}

// this step's weights as HL32 images + their scales; with `head` (fit steps) also the a-priori bound of the head's dz
struct HpHeadBoundArgs {
    const float* W;
    const float* b;
    const unsigned* tmax;
    const unsigned* wtmax;
    float inv_count, omega;
};
// x_measured: slots.x_max() holds max|x| of the rows this step runs on (the fit / forward entry points measure it first); false:
// the input is a coordinate grid or its Fourier features, |x| <= 1 (the dense re-sampling prepares the weights once per call,
// before any chunk's input exists)
static int hp_refresh_weights(const SplitCtx& c, const inr_siren_desc_t* d, const Layout& L, const float* params, hipStream_t st,
                              bool x_measured, const HpHeadBoundArgs* head = nullptr) {
    const float *W[HpSlots::MAX_LAYERS], *bias[HpSlots::MAX_LAYERS];
    float om[HpSlots::MAX_LAYERS];
    for (int l = 0; l < L.n_sine; ++l) {
        W[l] = params + L.w_off[l];
        bias[l] = params + L.b_off[l];
        om[l] = layer_omega(d, l);
    }
    return hp_weight_prep(W, L.fan_out.data(), L.fan_in.data(), L.n_sine, c.planes, c.slots, c.part,
                          head ? c.slots.head_bound() : nullptr, head ? head->W : nullptr, head ? head->b : nullptr,
                          L.fan_in[L.n_sine], head ? head->tmax : nullptr, head ? head->wtmax : nullptr,
                          head ? head->inv_count : 0.f, head ? head->omega : 0.f, st, bias, om, c.slots.act_bound(0),
                          x_measured ? c.slots.x_max() : nullptr);
}

static size_t head_backward_ws_floats(int64_t n, int hidden, int out_f) {
    const int64_t blocks = head_fused_blocks(n);
    const size_t fused = (size_t)(2 * blocks * hidden + reduce_tmp_floats(blocks, hidden) + 2 * blocks);   // + loss / sum-g partials
    const size_t a = (size_t)colsum_ws_floats(n, hidden, out_f);
    const size_t b = (size_t)colsum_ws_floats(n, out_f, 1);
    return max2(fused, max2(a, b));
}

// head backward: dz_last = (gy W) * dact_last, gW/gb of the head, and (optionally) gb_last = colsum(dz_last),
// the bias gradient of the last sine layer.  One fused pass when out_features == 1.
static int head_backward(float* dz_last, float* gW, float* gb, float* gb_last, const float* gy, const float* a_last,
                         const float* dact_last, const float* W, int64_t n, int hidden, int out_f, float* ws,
                         hipStream_t st, unsigned* dz_amax = nullptr) {
    if (dz_last && gW && dact_last && head_fused_ok(hidden, out_f, dz_last, a_last, dact_last, W)) {
        const int64_t blocks = head_fused_blocks(n);
        float* slab_b = ws;
        float* slab_w = ws + blocks * hidden;
        float* tmp = ws + 2 * blocks * hidden;
        if (int rc = launch_head_bwd_fused(dz_last, slab_b, slab_w, gy, W, a_last, dact_last, n, hidden, st, dz_amax))
            return rc;
        if (gb_last) {
            if (int rc = launch_reduce_slabs(gb_last, slab_b, (int)blocks, hidden, tmp, st)) return rc;
        }
        if (int rc = launch_reduce_slabs(gW, slab_w, (int)blocks, hidden, tmp, st)) return rc;
        if (gb) return launch_colsum(gb, gy, nullptr, n, out_f, 1, ws, st);
        return 0;
    }
    if (gW) {
        if (int rc = launch_colsum(gW, a_last, gy, n, hidden, out_f, ws, st)) return rc;
    }
    if (gb) {
        if (int rc = launch_colsum(gb, gy, nullptr, n, out_f, 1, ws, st)) return rc;
    }
    if (dz_last) {
        if (int rc = launch_head_dz(dz_last, gy, W, dact_last, n, hidden, out_f, st)) return rc;
        if (dz_amax) {
            if (int rc = h3_tensor_amax(dz_amax, dz_last, (long long)n * hidden, st)) return rc;
        }
        if (gb_last) return launch_colsum(gb_last, dz_last, nullptr, n, hidden, 1, ws, st);
    }
    return 0;
}

}  // namespace inr

using namespace inr;

extern "C" {

int inr_version(void) { return INR_ABI_VERSION; }
int inr_build_flags(void) { return gemm_build_flags(); }
const char* inr_last_error(void) { return g_err; }

int inr_device_caps(int device, inr_device_caps_t* out) {
    INR_REQUIRE(out != nullptr, INR_E_INVALID, "caps output is null");
    hipDeviceProp_t prop;
    INR_HIP(hipGetDeviceProperties(&prop, device));
    memset(out, 0, sizeof(*out));
    out->abi_version = INR_ABI_VERSION;
    out->device = device;
    out->compute_units = prop.multiProcessorCount;
    out->wavefront_size = prop.warpSize;
    out->lds_bytes_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    out->clock_khz = prop.clockRate;
    out->hbm_bytes = (int64_t)prop.totalGlobalMem;
    strncpy(out->arch, prop.gcnArchName, sizeof(out->arch) - 1);
    return 0;
}

// ---- layer-wise backward: head_backward, input_grad and param_grad above, which the fused fit shares ---------------------
size_t inr_head_backward_workspace_bytes(int64_t n, int hidden, int out_features) {
    return head_backward_ws_floats(n > 0 ? n : 1, hidden, out_features) * sizeof(float);
}

int inr_linear_head_backward(float* dz_last, float* gW, float* gb, float* gb_last, const float* gy,
                             const float* a_last, const float* dact_last, const float* W, int64_t n, int hidden,
                             int out_features, void* workspace, size_t workspace_bytes, void* stream) {
    INR_REQUIRE(gy && a_last && W, INR_E_INVALID, "inr_linear_head_backward: null pointer");
    INR_REQUIRE(n >= 1 && hidden >= 1 && out_features >= 1, INR_E_INVALID, "inr_linear_head_backward: bad sizes");
    INR_REQUIRE(workspace && workspace_bytes >= inr_head_backward_workspace_bytes(n, hidden, out_features),
                INR_E_WORKSPACE, "inr_linear_head_backward: workspace too small");
    INR_REQUIRE(!gb_last || dz_last, INR_E_INVALID, "inr_linear_head_backward: gb_last needs dz_last");
    return head_backward(dz_last, gW, gb, gb_last, gy, a_last, dact_last, W, n, hidden, out_features,
                         (float*)workspace, (hipStream_t)stream);
}

size_t inr_sine_layer_backward_input_workspace_bytes(int64_t n, int in_features) {
    return input_grad_ws_floats(n > 0 ? n : 1, in_features) * sizeof(float);
}

int inr_sine_layer_backward_input(float* dz_prev, float* gb_prev, const float* dz, const float* W,
                                  const float* dact_prev, int64_t n, int in_features, int out_features,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    INR_REQUIRE(dz_prev && dz && W, INR_E_INVALID, "inr_sine_layer_backward_input: null pointer");
    INR_REQUIRE(n >= 0 && n <= MAX_ROWS && in_features >= 1 && out_features >= 1, INR_E_INVALID,
                "inr_sine_layer_backward_input: bad sizes");
    if (n == 0) return 0;
    if (gb_prev)
        INR_REQUIRE(workspace && workspace_bytes >= inr_sine_layer_backward_input_workspace_bytes(n, in_features),
                    INR_E_WORKSPACE, "inr_sine_layer_backward_input: workspace too small for gb_prev");
    return input_grad(dz_prev, gb_prev, dz, W, dact_prev, n, in_features, out_features, (float*)workspace,
                      (hipStream_t)stream);
}

size_t inr_linear_param_grad_workspace_bytes(int64_t n, int in_features, int out_features) {
    return param_grad_ws_floats(n > 0 ? n : 1, in_features, out_features) * sizeof(float);
}

int inr_linear_param_grad(float* gW, float* gb, const float* dz, const float* x, int64_t n, int in_features,
                          int out_features, void* workspace, size_t workspace_bytes, void* stream) {
    INR_REQUIRE(gW && dz && x, INR_E_INVALID, "inr_linear_param_grad: null pointer");
    INR_REQUIRE(n >= 1 && n <= MAX_ROWS && in_features >= 1 && out_features >= 1, INR_E_INVALID,
                "inr_linear_param_grad: bad sizes");
    INR_REQUIRE(workspace && workspace_bytes >= inr_linear_param_grad_workspace_bytes(n, in_features, out_features),
                INR_E_WORKSPACE, "inr_linear_param_grad: workspace too small");
    return param_grad(gW, gb, dz, x, n, in_features, out_features, (float*)workspace, (hipStream_t)stream);
}

// ---- fused SIREN -------------------------------------------------------------------------------------
int64_t inr_siren_param_count(const inr_siren_desc_t* desc) {
    if (check_desc(desc)) return INR_E_INVALID;
    return make_layout(desc).total;
}

int inr_siren_param_offsets(const inr_siren_desc_t* desc, int64_t* offsets) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE(offsets != nullptr, INR_E_INVALID, "offsets is null");
    const Layout L = make_layout(desc);
    for (int l = 0; l <= L.n_sine; ++l) {
        offsets[2 * l] = L.w_off[l];
        offsets[2 * l + 1] = L.b_off[l];
    }
    return 0;
}

// ---- inference workspace: [feature buffer] | two activation buffers | split-GEMM context | HL32 image of the input --------------------
// The ONE place that sizes and carves it: inr_siren_forward (no feature buffer: x is the caller's) and inr_siren_reconstruct (one
// chunk of grid features).  workspace == nullptr: `total` only.
struct InferView {
    size_t total = 0;
    float* feats = nullptr;             // reconstruct only: fp32 features of one chunk
    float* buf[2] = {nullptr, nullptr}; // sine layers write them in turn
    SplitCtx ctx;
    char* xhl = nullptr;                // HL32 image of the input rows (pre-split path)
    bool hp = false;                    // the pre-split kernels serve this network
};
static InferView infer_view(const inr_siren_desc_t* d, const Layout& L, int64_t rows, bool with_feats, void* workspace) {
    InferView v;
    WsCarver c(workspace, 256);
    if (with_feats) v.feats = c.take<float>((size_t)rows * d->in_features);
    for (int k = 0; k < 2; ++k) v.buf[k] = c.take<float>((size_t)rows * d->hidden_features);
    char* ctx = c.take<char>(split_ctx_bytes(L));
    v.xhl = c.take<char>((size_t)rows * d->in_features * sizeof(float));
    v.total = c.bytes();
    if (!workspace) return v;
    v.ctx = split_ctx(L, ctx);
    v.hp = v.ctx.on && hp_eligible(d, L);
    return v;
}

size_t inr_siren_forward_workspace_bytes(const inr_siren_desc_t* desc, int64_t n) {
    if (check_desc(desc)) return 0;
    return infer_view(desc, make_layout(desc), n > 0 ? n : 1, false, nullptr).total;
}

// xhl_ready: the caller has already written the HL32 image of the input and its scale slot (hp_grid_fourier_hl); x unused
// amax_ready: the caller has measured max|x| into its slot (inr_siren_forward: before the weight preparation, which needs it)
static int siren_forward_impl(const inr_siren_desc_t* d, const Layout& L, const float* params, const float* x,
                              int64_t n, float* y, int use_clamp, float clamp_min, const InferView& v, hipStream_t st,
                              bool xhl_ready = false, bool amax_ready = false) {
    const SplitCtx& c = v.ctx;
    const float* cur = x;
    if (c.on && !xhl_ready && !amax_ready) {
        if (int rc = h3_tensor_amax(c.slots.x_max(), x, (long long)n * L.fan_in[0], st, 0x3f800000u)) return rc;
    }
    if (v.hp) {   // pre-split path: every activation lives in HBM as HL32 (gemm_hp.inc)
        if (!xhl_ready) {
            if (int rc = hp_convert(v.xhl, x, n, L.fan_in[0], c.x_scale(), st)) return rc;
        }
        if (hp_fused_forward_ok(L.fan_in[0], d->hidden_features, L.n_sine)) {
            // every sine layer and the head in ONE launch, the activations of a 64-row panel never leaving LDS (gemm_hp_fwd.inc)
            const char* W[HpSlots::MAX_LAYERS];
            const float* bias[HpSlots::MAX_LAYERS];
            const unsigned* wmax[HpSlots::MAX_LAYERS];
            for (int l = 0; l < L.n_sine; ++l) {
                W[l] = c.w_hl(l);
                bias[l] = params + L.b_off[l];
                wmax[l] = c.slots.w_max(l);
            }
            return hp_fused_forward(y, v.xhl, c.slots.x_max(), n, L.fan_in[0], d->hidden_features, L.n_sine, W, bias, wmax,
                                    d->first_omega, d->hidden_omega, params + L.w_off[L.n_sine], params + L.b_off[L.n_sine],
                                    use_clamp, clamp_min, st);
        }
        const char* in = v.xhl;
        for (int l = 0; l < L.n_sine; ++l) {
            char* dst = reinterpret_cast<char*>(v.buf[l & 1]);
            if (int rc = hp_sine_forward(dst, nullptr, in, c.w_hl(l), params + L.b_off[l], n, L.fan_in[l], L.fan_out[l],
                                         layer_omega(d, l), c.act_scale(l), c.w_scale(l), 0, st, false, c.act_scale(l + 1)))
                return rc;
            in = dst;
        }
        return hp_head_forward(y, in, params + L.w_off[L.n_sine], params + L.b_off[L.n_sine], n, d->hidden_features,
                               use_clamp, clamp_min, st, false, 0.f, c.act_scale(L.n_sine));
    }
    for (int l = 0; l < L.n_sine; ++l) {
        float* dst = v.buf[l & 1];
        H3Args ha;
        if (c.on) ha = h3_forward_args(c, l);
        if (int rc = gemm_sine_forward(dst, nullptr, cur, params + L.w_off[l], params + L.b_off[l], n, L.fan_in[l],
                                       L.fan_out[l], layer_omega(d, l), st, c.on ? &ha : nullptr))
            return rc;
        cur = dst;
    }
    return launch_head_forward(y, cur, params + L.w_off[L.n_sine], params + L.b_off[L.n_sine], n,
                               d->hidden_features, d->out_features, use_clamp, clamp_min, st);
}

int inr_siren_forward(const inr_siren_desc_t* desc, const float* params, const float* x, int64_t n, float* y,
                      int use_clamp, float clamp_min, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE(params && x && y, INR_E_INVALID, "inr_siren_forward: null pointer");
    INR_REQUIRE(n >= 0 && n <= MAX_ROWS, INR_E_INVALID, "inr_siren_forward: bad row count %lld", (long long)n);
    if (n == 0) return 0;
    const Layout L = make_layout(desc);
    const InferView v = infer_view(desc, L, n, false, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "inr_siren_forward: workspace too small");
    INR_REQUIRE(aligned16(workspace), INR_E_ALIGN, "inr_siren_forward: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (v.hp) {
        // max|x| first: the a-priori bounds of the layers' outputs (the scales of their images) start from it
        if (int rc = h3_tensor_amax(v.ctx.slots.x_max(), x, (long long)n * L.fan_in[0], st, 0x3f800000u)) return rc;
        if (int rc = hp_refresh_weights(v.ctx, desc, L, params, st, true)) return rc;
    } else if (v.ctx.on) {
        if (int rc = h3_refresh_weights(v.ctx, L, params, st)) return rc;
    }
    return siren_forward_impl(desc, L, params, x, n, y, use_clamp, clamp_min, v, st, false, v.hp);
}

size_t inr_siren_reconstruct_workspace_bytes(const inr_siren_desc_t* desc, int64_t chunk_rows) {
    if (check_desc(desc) || chunk_rows < 1) return 0;
    return infer_view(desc, make_layout(desc), chunk_rows, true, nullptr).total;
}

int inr_siren_reconstruct(const inr_siren_desc_t* desc, const float* params, const int64_t* shape, int dim,
                          const float* B, int m, float* y, int use_clamp, float clamp_min, int64_t chunk_rows,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE(params && shape && y, INR_E_INVALID, "inr_siren_reconstruct: null pointer");
    INR_REQUIRE(dim >= 1 && dim <= 8, INR_E_INVALID, "inr_siren_reconstruct: dim must be 1..8");
    INR_REQUIRE(chunk_rows >= 1 && chunk_rows <= MAX_ROWS, INR_E_INVALID, "inr_siren_reconstruct: bad chunk_rows");
    if (B)
        INR_REQUIRE(2 * m == desc->in_features, INR_E_INVALID,
                    "inr_siren_reconstruct: in_features (%d) must equal 2*m (%d)", desc->in_features, 2 * m);
    else
        INR_REQUIRE(dim == desc->in_features, INR_E_INVALID,
                    "inr_siren_reconstruct: without B the grid dim (%d) must equal in_features (%d)", dim,
                    desc->in_features);
    const Layout L = make_layout(desc);
    const InferView v = infer_view(desc, L, chunk_rows, true, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "inr_siren_reconstruct: workspace too small");
    INR_REQUIRE(aligned16(workspace), INR_E_ALIGN, "inr_siren_reconstruct: workspace must be 16-byte aligned");
    int64_t total = 1;
    for (int a = 0; a < dim; ++a) {
        INR_REQUIRE(shape[a] >= 1, INR_E_INVALID, "inr_siren_reconstruct: shape[%d] must be >= 1", a);
        total *= shape[a];
    }
    hipStream_t st = (hipStream_t)stream;
    if (v.hp) {
        if (int rc = hp_refresh_weights(v.ctx, desc, L, params, st, false)) return rc;
    } else if (v.ctx.on) {
        if (int rc = h3_refresh_weights(v.ctx, L, params, st)) return rc;
    }
    for (int64_t r0 = 0; r0 < total; r0 += chunk_rows) {
        const int64_t rows = (total - r0 < chunk_rows) ? (total - r0) : chunk_rows;
        // pre-split path with Fourier features: grid -> features -> HL32 image in ONE kernel (no fp32 feature matrix at all)
        const bool direct = v.hp && B && hp_grid_fourier_ok(m, dim);
        int rc = direct ? hp_grid_fourier_hl(v.xhl, v.ctx.slots.x_max(), shape, dim, r0, rows, B, m, st)
                 : B    ? launch_fourier(v.feats, nullptr, shape, dim, r0, rows, B, m, st)
                        : launch_mgrid(v.feats, shape, dim, r0, rows, st);
        if (rc) return rc;
        rc = siren_forward_impl(desc, L, params, v.feats, rows, y + r0 * desc->out_features, use_clamp, clamp_min, v, st, direct);
        if (rc) return rc;
    }
    return 0;
}

// ---- where the producers of the pre-split step leave their slab rows until launch_finalize sums them (common.h) ----------
// Tensor order = flat parameter order: W_0, b_0, ..., W_{S-1}, b_{S-1}, W_head, b_head.  Offsets in floats from the slab region.
struct HpSlabPlan {
    struct Seg {
        size_t slab, stage1;
        long long len;
        int max_rows;
    };
    std::vector<Seg> seg;       // 2 (S + 1)
    size_t part_loss = 0;       // [head blocks]
    size_t loss_sink = 0;       // where the loss goes when the caller does not want it
    size_t total = 0;
};
static HpSlabPlan hp_slab_plan(const Layout& L, int64_t n) {
    HpSlabPlan p;
    const int S = L.n_sine, H = L.fan_in[S];
    // rows of the head's slabs: one per block of hp_head_step_kernel, or two per 128-row panel when the head step rides in the last sine
    // layer's epilogue (hp_sine_forward_head) -- the plan reserves for whichever is more
    int64_t hb = hp_head_blocks(n);
    if (hp_row_head_rows(n) > hb) hb = hp_row_head_rows(n);
    WsCarver c(nullptr, 4 * sizeof(float));      // offsets only: the plan is in floats from the slab region
    auto here = [&] { return c.bytes() / sizeof(float); };
    auto add = [&](long long len, int rows) {
        HpSlabPlan::Seg sg;
        sg.len = len;
        sg.max_rows = rows;
        sg.slab = here();
        c.take<float>((size_t)rows * (size_t)len);
        sg.stage1 = here();
        if (rows > FIN_TALL) c.take<float>((size_t)((rows + FIN_GROUP - 1) / FIN_GROUP) * (size_t)len);
        p.seg.push_back(sg);
    };
    for (int l = 0; l < S; ++l) {
        add((long long)L.fan_in[l] * L.fan_out[l], hp_param_grad_splits(n, L.fan_in[l], L.fan_out[l]));
        add(L.fan_out[l], l == S - 1 ? (int)hb : hp_input_grad_max_rows(n));
    }
    add(H, (int)hb);     // W_head: the head step's slab_w
    add(1, (int)hb);     // b_head: its per-block sums of g
    p.part_loss = here();
    c.take<float>((size_t)hb);
    p.loss_sink = here();
    c.take<float>(4);
    p.total = here();
    return p;
}

// ---- fit workspace: acts (n_sine x n x H) | dacts (n_sine x n x H) | y | gy | scratch | split-GEMM context | HL32 image of x ---------
// The ONE place that sizes and carves it.  Every entry point that trains on a workspace (inr_siren_fit_cycle,
// inr_siren_loss_grad_ex, inr_siren_forward_train / inr_siren_backward_train) builds this view once per call, so the two passes of
// an autograd step see the same carve by construction.  workspace == nullptr: `total` only (the planner).  The fused
// small-network step carves the same bytes its own way (siren_small.hip); `total` covers it.
struct FitView {
    size_t total = 0;
    int64_t n = 0;
    std::vector<float*> act, dact;      // act[0] = x, act[l + 1] = output of sine layer l; dact[l]: its omega cos(.), later dz_l
    float *y = nullptr, *gy = nullptr;  // layer-wise path only
    float* scratch = nullptr;           // reduction workspaces of the layer-wise path / the slab region of the pre-split step
    SplitCtx ctx;
    char* xhl = nullptr;                // HL32 image of x (pre-split path)
    bool hp = false;                    // the pre-split kernels serve this network
    const char* act_hl(int l) const { return l == 0 ? xhl : reinterpret_cast<const char*>(act[l]); }
};
static FitView fit_view(const inr_siren_desc_t* d, const Layout& L, int64_t n, const float* x, void* workspace) {
    FitView v;
    v.n = n;
    size_t scratch = head_backward_ws_floats(n, d->hidden_features, d->out_features);
    for (int l = 0; l < L.n_sine; ++l) {
        scratch = max2(scratch, param_grad_ws_floats(n, L.fan_in[l], L.fan_out[l]));
        if (l > 0) scratch = max2(scratch, input_grad_ws_floats(n, L.fan_in[l]));
    }
    scratch = max2(scratch, (size_t)mse_blocks((int64_t)n * d->out_features) + 1);
    if (L.n_sine <= HpSlots::MAX_LAYERS && d->out_features == 1)
        scratch = max2(scratch, hp_slab_plan(L, n).total);   // deferred slabs of the HL32 step
    WsCarver c(workspace, 256);
    if (workspace) {
        v.act.resize(L.n_sine + 1);
        v.dact.resize(L.n_sine);
        v.act[0] = const_cast<float*>(x);
    }
    for (int k = 0; k < 2 * L.n_sine; ++k) {      // every layer's output, then every layer's dact
        float* a = c.take<float>((size_t)n * d->hidden_features);
        if (workspace) (k < L.n_sine ? v.act[k + 1] : v.dact[k - L.n_sine]) = a;
    }
    v.y = c.take<float>((size_t)n * d->out_features);
    v.gy = c.take<float>((size_t)n * d->out_features);
    v.scratch = c.take<float>(scratch);
    char* ctx = c.take<char>(split_ctx_bytes(L));
    v.xhl = c.take<char>((size_t)n * d->in_features * sizeof(float));
    v.total = c.bytes();
    if (small_path_ok(d, n)) {
        v.total = max2(v.total, round_up(small_workspace_floats(d, n, L.total) * sizeof(float), 256));
        if (small_multi_ok(d, n)) v.total = max2(v.total, round_up(small_multi_workspace_floats(d, n, L.total) * sizeof(float), 256));
    }
    if (!workspace) return v;
    v.ctx = split_ctx(L, ctx);
    v.hp = v.ctx.on && hp_eligible(d, L);
    return v;
}

// one forward (with stash) + loss + backward of the layer-wise path; grads land in the flat gradient buffer.
// count_total > 0: this is one row shard of a split fit (mean taken over count_total elements).
static int fit_forward_backward(const inr_siren_desc_t* d, const Layout& L, const float* params, float* grads, const FitView& v,
                                const float* target, const float* weight, int64_t count_total, float* loss_dst, hipStream_t st) {
    const int H = d->hidden_features, O = d->out_features, head = L.n_sine;
    const int64_t n = v.n;
    const std::vector<float*>&act = v.act, &dact = v.dact;
    float* scratch = v.scratch;
    const SplitCtx& c = v.ctx;
    const bool split = c.on;
    if (split) {   // this step's weights as fp16 planes; dz scale slots back to zero
        if (int rc = h3_refresh_weights(c, L, params, st)) return rc;
    }
    // forward with stash (SRDWI.py:58-59 per layer; dact = omega*cos(.) replaces autograd's saved z)
    for (int l = 0; l < L.n_sine; ++l) {
        H3Args ha;
        if (split) ha = h3_forward_args(c, l);
        if (int rc = gemm_sine_forward(act[l + 1], dact[l], act[l], params + L.w_off[l], params + L.b_off[l], n,
                                       L.fan_in[l], L.fan_out[l], layer_omega(d, l), st, split ? &ha : nullptr))
            return rc;
    }
    // head forward, loss + dL/dy (superresDWI.py:135), head backward; then the sine layers from last to first, dz
    // overwriting dact in place (bias gradients ride along: the head pass yields gb of the last sine layer, every
    // input-grad GEMM yields gb of the layer below from its epilogue)
    unsigned* dz_amax = split ? c.slots.dz_max(head - 1) : nullptr;
    if (head_step_fused_ok(H, O, act[head], dact[head - 1], params + L.w_off[head], scratch)) {
        // one pass over act_L / dact_L does all three (kernels.hip: head_step_fused_kernel)
        const int64_t blocks = head_fused_blocks(n);
        float* slab_b = scratch;
        float* slab_w = scratch + blocks * H;
        float* tmp = scratch + 2 * blocks * H;
        float* part_loss = tmp + reduce_tmp_floats(blocks, H);
        float* part_g = part_loss + blocks;
        if (int rc = launch_head_step_fused(dact[head - 1], slab_b, slab_w, part_loss, part_g, act[head], dact[head - 1],
                                            params + L.w_off[head], params + L.b_off[head], target, weight, n, H,
                                            count_total, st, dz_amax))
            return rc;
        if (int rc = launch_reduce_slabs(grads + L.b_off[head - 1], slab_b, (int)blocks, H, tmp, st)) return rc;
        if (int rc = launch_reduce_slabs(grads + L.w_off[head], slab_w, (int)blocks, H, tmp, st)) return rc;
        const float inv = (float)(1.0 / (double)(count_total > 0 ? count_total : n));
        if (int rc = launch_finish_sum(loss_dst, part_loss, (int)blocks, inv, st)) return rc;
        if (int rc = launch_finish_sum(grads + L.b_off[head], part_g, (int)blocks, 1.0f, st)) return rc;
    } else {
        if (int rc = launch_head_forward(v.y, act[head], params + L.w_off[head], params + L.b_off[head], n, H, O, 0,
                                         0.f, st))
            return rc;
        if (int rc = launch_mse(v.gy, loss_dst, v.y, target, weight, n * O, scratch + 1, st, count_total)) return rc;
        if (int rc = head_backward(dact[head - 1], grads + L.w_off[head], grads + L.b_off[head],
                                   grads + L.b_off[head - 1], v.gy, act[head], dact[head - 1], params + L.w_off[head], n,
                                   H, O, scratch, st, dz_amax))
            return rc;
    }
    for (int l = L.n_sine - 1; l >= 0; --l) {
        H3Args hp, hi;
        if (split) {
            hp = h3_param_grad_args(c, l);
            if (l > 0) hi = h3_input_grad_args(c, l);
        }
        if (int rc = param_grad(grads + L.w_off[l], nullptr, dact[l], act[l], n, L.fan_in[l], L.fan_out[l],
                                scratch, st, split ? &hp : nullptr))
            return rc;
        if (l > 0) {
            if (int rc = input_grad(dact[l - 1], grads + L.b_off[l - 1], dact[l], params + L.w_off[l], dact[l - 1],
                                    n, L.fan_in[l], L.fan_out[l], scratch, st, split ? &hi : nullptr))
                return rc;
        }
    }
    return 0;
}


// ---- the parameter-gradient GEMMs of a step below 200,000 rows: one launch for all layers (inr_debug_set(20, 0): one per layer) --
// dW_l = dz_l^T act_l depends on the stashed activations and on dz_l only: all of them can wait until the input-gradient chain
// has produced every dz, and then run as ONE launch (gemm_hp_rc_multi_kernel) whose row splits are chosen for the launch as a
// whole -- one round of blocks over the chip -- instead of for every layer alone.  A rocprofv3 timeline of a 4,096-row step
// (tools/kt_timeline.py) had shown four 13-20 us launches that each fill half the chip, 28 us of event hand-shakes of the first
// form of this switch (a second stream), and 16 row splits per layer = 448 blocks writing 57 MB of slabs for `finalize` to read
// back.  Measured, ms per step, one launch per layer / merged (tools/side_stream_ab.py): 2,048 rows 0.182 / 0.146, 4,096: 0.216
// / 0.181, 8,192: 0.325 / 0.277, 16,384: 0.454 / 0.381, 32,768: 0.674 / 0.630, 69,632: 1.318 / 1.279, 139,264: 2.431 / 2.408,
// 262,144: 4.42 / 4.42.  (The last bits of the gradients differ between the two forms: other row ranges per partial sum.)
static tune_int g_hp_side_stream{1};   // (the name of the first form; key 20) identical bits either way
static tune_int g_hp_merge_blocks{256};  // key 22: block count the merged parameter-gradient launch aims at (row splits = this / tiles)

// the same step on the pre-split path (gemm_hp.inc): act[l] (l >= 1) and dz are HL32, act[0] = the HL32 image of x,
// dact fp32 until the backward pass overwrites it with dz (HL32, scaled from an a-priori bound).
// forward of the sine layers (stash kept for the backward pass); z_head: the last layer stashes z + b only (HPE_Z)
// skip_last: the last sine layer runs inside hp_backward_pass with the head step in its epilogue (hp_sine_forward_head)
static int hp_forward_pass(const inr_siren_desc_t* d, const Layout& L, const float* params, const FitView& v, hipStream_t st,
                           bool z_head, bool skip_last = false) {
    const SplitCtx& c = v.ctx;
    const int head = L.n_sine;
    for (int l = 0; l < L.n_sine - (skip_last ? 1 : 0); ++l) {
        if (int rc = hp_sine_forward(reinterpret_cast<char*>(v.act[l + 1]), v.dact[l], v.act_hl(l), c.w_hl(l), params + L.b_off[l],
                                     v.n, L.fan_in[l], L.fan_out[l], layer_omega(d, l), c.act_scale(l), c.w_scale(l), 0, st,
                                     z_head && l == head - 1, c.act_scale(l + 1)))
            return rc;
    }
    return 0;
}

// head step + backward of every layer.  The loss gradient is formed here from (target, weight) -- the fused fit -- or taken from
// the caller (g_ext = dL/dy, the autograd path; target / weight unused, no loss).  Gradients are NOT reduced here: every producer
// leaves its slab rows in v.scratch and `fin` describes them (the caller finishes with launch_finalize).
static int hp_backward_pass(const inr_siren_desc_t* d, const Layout& L, const float* params, float* grads, const FitView& v,
                            const float* target, const float* weight, const float* g_ext, int64_t count_total, float* loss_dst,
                            hipStream_t st, FinalizeJob& fin, bool z_head, bool fuse_head = false) {
    const int H = d->hidden_features, head = L.n_sine;
    const int64_t n = v.n;
    const SplitCtx& c = v.ctx;
    float* slabs = v.scratch;
    const HpSlabPlan plan = hp_slab_plan(L, n);
    const float inv = (float)(1.0 / (double)(count_total > 0 ? count_total : n));
    const float omega_last = layer_omega(d, head - 1);
    fin = FinalizeJob{};
    fin.nseg = 2 * (head + 1);
    for (int k = 0; k < fin.nseg; ++k) {
        const int l = k >> 1;
        fin.seg[k].slab = slabs + plan.seg[k].slab;
        fin.seg[k].stage1 = slabs + plan.seg[k].stage1;
        fin.seg[k].len = plan.seg[k].len;
        fin.seg[k].dst = (k & 1) ? L.b_off[l] : L.w_off[l];
        fin.seg[k].nslabs = 0;
    }
    fin.grads = grads;
    fin.loss_out = loss_dst;
    fin.loss_scale = inv;
    auto slab_of = [&](int k) { return slabs + plan.seg[k].slab; };
    // scale of dz_l: the head's bound for the last sine layer, else measured max|dz_{l+1}| * wnorm_{l+1} * omega_l
    auto dz_scale = [&](int l) {
        HpScale s;
        if (l == head - 1) {
            s.wn = c.slots.head_bound();
            s.mul = 1.f;
        } else {
            s.meas = c.slots.dz_max(l + 1);
            s.wn = c.slots.wnorm(l + 1);
            s.mul = fabsf(layer_omega(d, l)) * 1.001f;
        }
        return s;
    };
    {   // the head step: dz of the last sine layer + the slab rows of b_{S-1}, W_head, b_head and of the loss
        const int kb = 2 * (head - 1) + 1, kw = 2 * head, kg = 2 * head + 1;
        float* part_loss = slabs + plan.part_loss;
        char* dz_hl = reinterpret_cast<char*>(v.dact[head - 1]);
        int rows;
        if (fuse_head) {   // in the last sine layer's epilogue: no z round trip, no head step kernel (gemm_hp_row.inc, HPE_HEAD)
            rows = hp_row_head_rows(n);
            if (int rc = hp_sine_forward_head(dz_hl, v.act_hl(head - 1), c.w_hl(head - 1), params + L.b_off[head - 1], n,
                                              L.fan_in[head - 1], H, omega_last, c.act_scale(head - 1), c.w_scale(head - 1),
                                              dz_scale(head - 1), params + L.w_off[head], params + L.b_off[head], target, weight,
                                              count_total, slab_of(kb), slab_of(kw), part_loss, slab_of(kg),
                                              c.slots.dz_max(head - 1), st))
                return rc;
        } else {
            rows = (int)hp_head_blocks(n);
            if (int rc = hp_head_step(dz_hl, slab_of(kb), slab_of(kw), part_loss, slab_of(kg), v.act_hl(head), v.dact[head - 1],
                                      params + L.w_off[head], params + L.b_off[head], target, weight, n, H, count_total,
                                      c.slots.dz_max(head - 1), dz_scale(head - 1), st, z_head, omega_last, g_ext,
                                      c.act_scale(head)))
                return rc;
        }
        fin.seg[kb].nslabs = fin.seg[kw].nslabs = fin.seg[kg].nslabs = rows;
        fin.part_loss = part_loss;
        fin.nparts = rows;
    }
    // (only where it pays: see above)
    const bool merge = g_hp_side_stream && L.n_sine > 1 && n < 200000 && L.n_sine <= hp_param_grad_multi_max();
    HpParamGradJob jobs[16];
    int njobs = 0;
    // merged: the launch as a whole should be ONE round of blocks over the chip -- row splits for that, not for each layer alone
    // (at 4,096 rows 16 splits per layer made 448 blocks that wrote 57 MB of slabs for `finalize` to read back; 9 make 252 and 32)
    int merged_splits = 1 << 30;
    if (merge) {
        long long tiles_all = 0;
        for (int l = 0; l < L.n_sine; ++l) tiles_all += (long long)((L.fan_out[l] + 127) / 128) * ((L.fan_in[l] + 255) / 256);
        const int target = g_hp_merge_blocks;
        merged_splits = (int)(target / tiles_all > 1 ? target / tiles_all : 1);
        const int min_by_len = (int)((n + 16383) / 16384);      // (hp_param_grad_splits: no register accumulation over > 16 k rows)
        if (merged_splits < min_by_len) merged_splits = min_by_len;
    }
    for (int l = L.n_sine - 1; l >= 0; --l) {
        const char* dz = reinterpret_cast<const char*>(v.dact[l]);
        int splits = hp_param_grad_splits(n, L.fan_in[l], L.fan_out[l]);     // (what the slab plan reserves: an upper bound)
        if (splits > merged_splits) splits = merged_splits;
        if (merge) {
            jobs[njobs++] = HpParamGradJob{slab_of(2 * l), splits, dz, v.act_hl(l), L.fan_in[l], L.fan_out[l], dz_scale(l),
                                           c.act_scale(l)};
        } else if (int rc = hp_param_grad_slabs(slab_of(2 * l), splits, dz, v.act_hl(l), n, L.fan_in[l], L.fan_out[l], dz_scale(l),
                                                c.act_scale(l), st)) {
            return rc;
        }
        fin.seg[2 * l].nslabs = splits;
        if (l > 0) {
            int rows = 0;
            if (int rc = hp_input_grad(reinterpret_cast<char*>(v.dact[l - 1]), dz, c.wT_hl(l), v.dact[l - 1], n, L.fan_in[l],
                                       L.fan_out[l], slab_of(2 * (l - 1) + 1), &rows, c.slots.dz_max(l - 1), dz_scale(l),
                                       c.w_scale(l), dz_scale(l - 1), st))
                return rc;
            fin.seg[2 * (l - 1) + 1].nslabs = rows;
        }
    }
    if (merge) {
        if (int rc = hp_param_grad_multi(jobs, njobs, n, st)) return rc;
    }
    return 0;
}

static int fit_forward_backward_hp(const inr_siren_desc_t* d, const Layout& L, const float* params, float* grads, const FitView& v,
                                   const float* target, const float* weight, int64_t count_total, float* loss_dst, hipStream_t st,
                                   FinalizeJob& fin) {
    const int head = L.n_sine;
    const HpSlots& s = v.ctx.slots;
    const float inv = (float)(1.0 / (double)(count_total > 0 ? count_total : v.n));
    const HpHeadBoundArgs hb{params + L.w_off[head], params + L.b_off[head], s.target_max(), weight ? s.weight_max() : nullptr,
                             inv, layer_omega(d, head - 1)};
    if (int rc = hp_refresh_weights(v.ctx, d, L, params, st, true, &hb)) return rc;
    // the output of the LAST sine layer feeds nothing but the head: that layer stashes z + b only (one fp32 matrix instead
    // of act + omega cos) and the head step forms sin / cos itself -- 2.1 GB less HBM traffic per step at N = 524,288
    const bool z_head = hp_z_stash_ok(L.fan_in[head - 1]);
    // ... and from 768 row panels (98,304 rows) on the head step rides in that layer's epilogue (a block of gemm_hp_row_kernel owns whole rows)
    const bool fuse_head = z_head && hp_row_head_ok(v.n, d->hidden_features, L.fan_in[head - 1]);
    if (int rc = hp_forward_pass(d, L, params, v, st, z_head, fuse_head)) return rc;
    return hp_backward_pass(d, L, params, grads, v, target, weight, nullptr, count_total, loss_dst, st, fin, z_head, fuse_head);
}

// max|x| of this call's rows into its slot (floor 1: see h3_tensor_amax)
static int measure_x(const FitView& v, const Layout& L, hipStream_t st) {
    return h3_tensor_amax(v.ctx.slots.x_max(), v.act[0], (long long)v.n * L.fan_in[0], st, 0x3f800000u);
}
// per call: scales of the targets (several acquisitions behind one pointer: the bounds cover all of them), HL32 image of x.
// keep_stats / keep_x: they are the previous call's (the caller vouches for it: see ReuseStamp)
static int hp_prepare_call(const FitView& v, const Layout& L, const float* target, const float* weight, int out_f, hipStream_t st,
                           int64_t n_acq = 1, bool keep_x = false, bool keep_stats = false) {
    const HpSlots& s = v.ctx.slots;
    if (!keep_stats) {
        if (int rc = h3_tensor_amax(s.target_max(), target, (long long)v.n * n_acq * out_f, st, 0u)) return rc;
        if (weight) {
            if (int rc = h3_tensor_amax(s.weight_max(), weight, (long long)v.n * n_acq * out_f, st, 0u)) return rc;
        }
    }
    if (keep_x) return 0;
    return hp_convert(v.xhl, v.act[0], v.n, L.fan_in[0], v.ctx.x_scale(), st);
}

// What the last inr_siren_loss_grad_ex call left in a workspace, remembered on the HOST (the call must not sync to look into the
// device bytes): a REUSE flag is honoured only when this call's (n, fan_in, x) -- and (target, weight) for the statistics -- are
// the ones the image / slots in that workspace were built from.  A wrong flag (first call, another n, another x) used to run on
// stale or uninitialised operand images and return wrong gradients with rc 0.
namespace {
struct ReuseStamp {
    const void* ws = nullptr;
    int64_t n = 0;
    int fan_in = 0;
    const void *x = nullptr, *target = nullptr, *weight = nullptr;
    bool image = false, stats = false;
    bool fwd_train = false;      // an inr_siren_forward_train stash is pending (inr_siren_backward_train consumes it)
    unsigned long long used = 0; // last use (least recently used entry is replaced)
    bool holds_image(int64_t n_, int fan_in_, const void* x_) const { return image && n == n_ && fan_in == fan_in_ && x == x_; }
    bool holds_stats(int64_t n_, const void* t, const void* w) const { return stats && n == n_ && target == t && weight == w; }
};
std::mutex g_reuse_mu;
ReuseStamp g_reuse[64];
unsigned long long g_reuse_next = 0;
ReuseStamp* reuse_find(const void* ws, bool create) {      // (caller holds g_reuse_mu)
    for (auto& s : g_reuse)
        if (s.ws == ws) {
            s.used = ++g_reuse_next;
            return &s;
        }
    if (!create) return nullptr;
    ReuseStamp* lru = &g_reuse[0];                          // the least recently used entry makes room
    for (auto& s : g_reuse)
        if (s.used < lru->used) lru = &s;
    *lru = ReuseStamp{};
    lru->ws = ws;
    lru->used = ++g_reuse_next;
    return lru;
}
// a call is about to rebuild the operand image and the statistics slots of this workspace: a later REUSE flag must not trust them
void reuse_invalidate(const void* ws) {
    std::lock_guard<std::mutex> lk(g_reuse_mu);
    if (ReuseStamp* s = reuse_find(ws, false)) s->image = s->stats = s->fwd_train = false;
}
}   // namespace

size_t inr_siren_fit_workspace_bytes(const inr_siren_desc_t* desc, int64_t n) {
    if (check_desc(desc) || n < 1) return 0;
    return fit_view(desc, make_layout(desc), n, nullptr, nullptr).total;
}

int inr_siren_fit(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                  const float* target, const float* weight, int64_t n, int64_t first_step, int n_steps, double lr,
                  double beta1, double beta2, double eps, float* losses, void* workspace, size_t workspace_bytes,
                  void* stream) {
    return inr_siren_fit_cycle(desc, params, grads, m, v, x, target, weight, 1, 0, n, first_step, n_steps, lr, beta1, beta2,
                               eps, losses, workspace, workspace_bytes, stream);
}

int inr_siren_fit_cycle(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                        const float* targets, const float* weights, int n_acq, int first_acq, int64_t n,
                        int64_t first_step, int n_steps, double lr, double beta1, double beta2, double eps, float* losses,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE(params && grads && m && v && x && targets, INR_E_INVALID, "inr_siren_fit: null pointer");
    INR_REQUIRE(n >= 1 && n <= MAX_ROWS, INR_E_INVALID, "inr_siren_fit: bad row count %lld", (long long)n);
    INR_REQUIRE(first_step >= 1 && n_steps >= 0, INR_E_INVALID, "inr_siren_fit: first_step >= 1, n_steps >= 0");
    INR_REQUIRE(n_acq >= 1 && first_acq >= 0 && first_acq < n_acq, INR_E_INVALID,
                "inr_siren_fit_cycle: need n_acq >= 1 and 0 <= first_acq < n_acq");
    const int64_t acq_stride = n * desc->out_features;      // floats between consecutive acquisitions
    const Layout L = make_layout(desc);
    const FitView fv = fit_view(desc, L, n, x, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= fv.total, INR_E_WORKSPACE,
                "inr_siren_fit: workspace too small (%zu < %zu)", workspace_bytes, fv.total);
    INR_REQUIRE(aligned16(workspace) && aligned16(params) && aligned16(grads) && aligned16(x), INR_E_ALIGN,
                "inr_siren_fit: params/grads/x/workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    reuse_invalidate(workspace);
    if (small_path_ok(desc, n) && !g_force_generic) {
        // master.py regime (small network, few thousand rows): one fused forward+backward launch + one reduce/Adam
        // launch per step instead of ~45 layer-wise launches (csrc/siren_small.hip)
        if (g_small_multi && small_multi_ok(desc, n)) {   // all steps inside one persistent launch per 64 steps
            const int rc = small_fit_multi(desc, L.w_off.data(), L.b_off.data(), L.total, params, grads, m, v, x, targets, weights,
                                           n_acq, first_acq, n, first_step, n_steps, lr, beta1, beta2, eps, losses,
                                           (float*)workspace, st);
            if (rc != INR_E_FALLBACK) return rc;   // (a device that cannot hold the grid co-resident: two launches per step)
        }
        for (int it = 0; it < n_steps; ++it) {
            const int64_t a = (first_acq + it) % n_acq;
            if (int rc = small_fit_step(desc, L.w_off.data(), L.b_off.data(), L.total, params, grads, m, v, x,
                                        targets + a * acq_stride, weights ? weights + a * acq_stride : nullptr, n,
                                        first_step + it, lr, beta1, beta2, eps, losses ? losses + it : nullptr,
                                        (float*)workspace, st))
                return rc;
        }
        return 0;
    }

    if (fv.ctx.on) {
        if (int rc = measure_x(fv, L, st)) return rc;
    }
    // where the loss goes when the caller does not want it: a word the step overwrites later (layer-wise path), or the plan's own
    // (pre-split path: scratch[0] is a slab row the finalize launch still reads)
    float* loss_sink = fv.hp ? fv.scratch + hp_slab_plan(L, n).loss_sink : fv.scratch;
    if (fv.hp && n_steps > 0) {
        if (int rc = hp_prepare_call(fv, L, targets, weights, desc->out_features, st, n_acq)) return rc;
    }
    for (int it = 0; it < n_steps; ++it) {
        const int64_t a = (first_acq + it) % n_acq;
        const float* target = targets + a * acq_stride;
        const float* weight = weights ? weights + a * acq_stride : nullptr;
        float* loss_dst = losses ? (losses + it) : loss_sink;
        if (fv.hp) {   // gradient sums, loss and the Adam step in one launch behind the backward pass
            FinalizeJob fin;
            if (int rc = fit_forward_backward_hp(desc, L, params, grads, fv, target, weight, 0, loss_dst, st, fin)) return rc;
            fin.params = params;
            fin.m = m;
            fin.v = v;
            if (int rc = launch_finalize(fin, first_step + it, lr, beta1, beta2, eps, st)) return rc;
            continue;
        }
        if (int rc = fit_forward_backward(desc, L, params, grads, fv, target, weight, 0, loss_dst, st)) return rc;
        if (int rc = launch_adam(params, grads, m, v, L.total, first_step + it, lr, beta1, beta2, eps, st)) return rc;
    }
    return 0;
}

// n_fits independent fits of one shape, equivalent bit for bit to inr_siren_fit_cycle(fit 0), (fit 1), ... on `stream`.  Fits
// the persistent kernel serves, and of which at least two fit one cooperative grid, share launches (small_fit_batch); every
// other case is that sequence of solo calls.
int inr_siren_fit_cycle_batch(const inr_siren_desc_t* desc, int n_fits, float* const* params, float* const* grads,
                              float* const* m, float* const* v, const float* x, const float* const* targets,
                              const float* const* weights, const int* n_acq, const int* first_acq, int64_t n, int64_t first_step,
                              int n_steps, double lr, double beta1, double beta2, double eps, float* const* losses,
                              void* const* workspaces, size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE(n_fits >= 1, INR_E_INVALID, "inr_siren_fit_cycle_batch: n_fits must be >= 1 (got %d)", n_fits);
    INR_REQUIRE(params && grads && m && v && targets && n_acq && first_acq && workspaces, INR_E_INVALID,
                "inr_siren_fit_cycle_batch: null array (params, grads, m, v, targets, n_acq, first_acq and workspaces are "
                "required; weights and losses may be null)");
    INR_REQUIRE(x != nullptr, INR_E_INVALID, "inr_siren_fit_cycle_batch: x is null");
    INR_REQUIRE(n >= 1 && n <= MAX_ROWS, INR_E_INVALID, "inr_siren_fit_cycle_batch: bad row count %lld", (long long)n);
    INR_REQUIRE(first_step >= 1 && n_steps >= 0, INR_E_INVALID, "inr_siren_fit_cycle_batch: first_step >= 1, n_steps >= 0");
    INR_REQUIRE(aligned16(x), INR_E_INVALID, "inr_siren_fit_cycle_batch: x is not 16-byte aligned");
    for (int i = 0; i < n_fits; ++i) {
        INR_REQUIRE(params[i] && grads[i] && m[i] && v[i] && targets[i] && workspaces[i], INR_E_INVALID,
                    "inr_siren_fit_cycle_batch: fit %d has a null params / grads / m / v / targets / workspace pointer", i);
        INR_REQUIRE(aligned16(params[i]) && aligned16(grads[i]) && aligned16(workspaces[i]), INR_E_INVALID,
                    "inr_siren_fit_cycle_batch: fit %d: params / grads / workspace are not 16-byte aligned", i);
        INR_REQUIRE(n_acq[i] >= 1 && first_acq[i] >= 0 && first_acq[i] < n_acq[i], INR_E_INVALID,
                    "inr_siren_fit_cycle_batch: fit %d: need n_acq >= 1 and 0 <= first_acq < n_acq (got n_acq %d, first_acq %d)",
                    i, n_acq[i], first_acq[i]);
        for (int j = 0; j < i; ++j) {
            INR_REQUIRE(params[j] != params[i], INR_E_INVALID, "inr_siren_fit_cycle_batch: fits %d and %d share one params buffer",
                        j, i);
            INR_REQUIRE(workspaces[j] != workspaces[i], INR_E_INVALID,
                        "inr_siren_fit_cycle_batch: fits %d and %d share one workspace", j, i);
        }
    }
    const Layout L = make_layout(desc);
    const size_t need = fit_view(desc, L, n, nullptr, nullptr).total;
    INR_REQUIRE(workspace_bytes >= need, INR_E_WORKSPACE, "inr_siren_fit_cycle_batch: workspace too small (%zu < %zu)",
                workspace_bytes, need);
    if (small_path_ok(desc, n) && !g_force_generic && g_small_multi && small_batch_per_launch(desc, n) >= 2) {
        for (int i = 0; i < n_fits; ++i) reuse_invalidate(workspaces[i]);      // (as in inr_siren_fit_cycle)
        const int rc = small_fit_batch(desc, L.w_off.data(), L.b_off.data(), L.total, n_fits, params, grads, m, v, x, targets,
                                       weights, n_acq, first_acq, n, first_step, n_steps, lr, beta1, beta2, eps, losses,
                                       workspaces, (hipStream_t)stream);
        if (rc != INR_E_FALLBACK) return rc;   // (the device refused the first grid: the solo calls below)
    }
    for (int i = 0; i < n_fits; ++i) {
        if (int rc = inr_siren_fit_cycle(desc, params[i], grads[i], m[i], v[i], x, targets[i], weights ? weights[i] : nullptr,
                                         n_acq[i], first_acq[i], n, first_step, n_steps, lr, beta1, beta2, eps,
                                         losses ? losses[i] : nullptr, workspaces[i], workspace_bytes, stream))
            return rc;
    }
    return 0;
}

// forward + loss + backward only (no optimizer): the building block of a fit whose rows are split over GPUs
int inr_siren_loss_grad(const inr_siren_desc_t* desc, const float* params, float* grads, const float* x,
                        const float* target, const float* weight, int64_t n, int64_t count_total, float* loss,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return inr_siren_loss_grad_ex(desc, params, grads, x, target, weight, n, count_total, loss, workspace, workspace_bytes, 0,
                                  stream);
}


int inr_siren_loss_grad_ex(const inr_siren_desc_t* desc, const float* params, float* grads, const float* x,
                           const float* target, const float* weight, int64_t n, int64_t count_total, float* loss,
                           void* workspace, size_t workspace_bytes, int flags, void* stream) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE((flags & ~(INR_REUSE_INPUT_IMAGE | INR_REUSE_TARGET_STATS)) == 0, INR_E_INVALID,
                "inr_siren_loss_grad_ex: unknown flags 0x%x", flags);
    INR_REQUIRE(params && grads && x && target && loss, INR_E_INVALID, "inr_siren_loss_grad: null pointer");
    INR_REQUIRE(n >= 1 && n <= MAX_ROWS, INR_E_INVALID, "inr_siren_loss_grad: bad row count %lld", (long long)n);
    INR_REQUIRE(count_total == 0 || count_total >= n * desc->out_features, INR_E_INVALID,
                "inr_siren_loss_grad: count_total must be 0 or >= n*out_features");
    const Layout L = make_layout(desc);
    const FitView fv = fit_view(desc, L, n, x, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= fv.total, INR_E_WORKSPACE,
                "inr_siren_loss_grad: workspace too small (%zu < %zu)", workspace_bytes, fv.total);
    INR_REQUIRE(aligned16(workspace) && aligned16(params) && aligned16(grads) && aligned16(x), INR_E_ALIGN,
                "inr_siren_loss_grad: params/grads/x/workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    // A network the pre-split kernels do not serve keeps no operand image and no target statistics in its workspace: there is
    // nothing a REUSE flag could refer to, so the flags are accepted and mean nothing (round 5: they were REFUSED, which made every
    // multi-step ShardedSirenFitter.step on e.g. Siren(32, 64, 1, 1) fail at its second step -- found by tests/test_gpu_nccl.py).
    if (!fv.hp) flags = 0;
    const bool keep_x = (flags & INR_REUSE_INPUT_IMAGE) != 0, keep_stats = (flags & INR_REUSE_TARGET_STATS) != 0;
    {
        std::lock_guard<std::mutex> lk(g_reuse_mu);
        ReuseStamp* s = reuse_find(workspace, flags == 0);
        if (keep_x)
            INR_REQUIRE(s && s->holds_image(n, L.fan_in[0], x), INR_E_INVALID,
                        "inr_siren_loss_grad_ex: INR_REUSE_INPUT_IMAGE, but this workspace does not hold the image of these %lld rows of x",
                        (long long)n);
        if (keep_stats)
            INR_REQUIRE(s && s->holds_stats(n, target, weight), INR_E_INVALID,
                        "inr_siren_loss_grad_ex: INR_REUSE_TARGET_STATS, but this workspace does not hold the statistics of this target");
        if (!s) s = reuse_find(workspace, true);
        if (!keep_x) { s->image = fv.hp; s->x = x; s->fan_in = L.fan_in[0]; }
        if (!keep_stats) { s->stats = fv.hp; s->target = target; s->weight = weight; }
        s->n = n;
    }
    if (fv.ctx.on && !keep_x) {
        if (int rc = measure_x(fv, L, st)) return rc;
    }
    if (fv.hp) {
        if (int rc = hp_prepare_call(fv, L, target, weight, desc->out_features, st, 1, keep_x, keep_stats)) return rc;
        FinalizeJob fin;
        if (int rc = fit_forward_backward_hp(desc, L, params, grads, fv, target, weight, count_total, loss, st, fin)) return rc;
        return launch_finalize(fin, 0, 0.0, 0.0, 0.0, 0.0, st);
    }
    return fit_forward_backward(desc, L, params, grads, fv, target, weight, count_total, loss, st);
}

// ---- the autograd path on the fused fit's kernels (include/inrhip.h (f)) ------------------------------------------------------
int inr_siren_hp_eligible(const inr_siren_desc_t* desc) {
    if (check_desc(desc)) return 0;
    const Layout L = make_layout(desc);
    return hp_eligible(desc, L) ? 1 : 0;
}

int inr_siren_forward_train(const inr_siren_desc_t* desc, const float* params, const float* x, float* y, int64_t n,
                            void* workspace, size_t workspace_bytes, int flags, void* stream) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE((flags & ~INR_REUSE_INPUT_IMAGE) == 0, INR_E_INVALID, "inr_siren_forward_train: unknown flags 0x%x", flags);
    INR_REQUIRE(params && x && y, INR_E_INVALID, "inr_siren_forward_train: null pointer");
    INR_REQUIRE(n >= 1 && n <= MAX_ROWS, INR_E_INVALID, "inr_siren_forward_train: bad row count %lld", (long long)n);
    const Layout L = make_layout(desc);
    INR_REQUIRE(hp_eligible(desc, L), INR_E_INVALID, "inr_siren_forward_train: network shape not served by the pre-split kernels "
                "(ask inr_siren_hp_eligible)");
    INR_REQUIRE(aligned16(workspace) && aligned16(params) && aligned16(x), INR_E_ALIGN,
                "inr_siren_forward_train: params/x/workspace must be 16-byte aligned");
    const FitView fv = fit_view(desc, L, n, x, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= fv.total, INR_E_WORKSPACE,
                "inr_siren_forward_train: workspace too small (%zu < %zu)", workspace_bytes, fv.total);
    hipStream_t st = (hipStream_t)stream;
    const bool keep_x = (flags & INR_REUSE_INPUT_IMAGE) != 0;
    {
        std::lock_guard<std::mutex> lk(g_reuse_mu);
        ReuseStamp* s = reuse_find(workspace, !keep_x);
        if (keep_x)
            INR_REQUIRE(s && s->holds_image(n, L.fan_in[0], x), INR_E_INVALID,
                        "inr_siren_forward_train: INR_REUSE_INPUT_IMAGE, but this workspace does not hold the image of these %lld rows of x",
                        (long long)n);
        s->image = true;
        s->x = x;
        s->fan_in = L.fan_in[0];
        s->n = n;
        s->stats = false;
        s->fwd_train = true;
    }
    if (!keep_x) {
        if (int rc = measure_x(fv, L, st)) return rc;
        if (int rc = hp_convert(fv.xhl, x, n, L.fan_in[0], fv.ctx.x_scale(), st)) return rc;
    }
    if (int rc = hp_refresh_weights(fv.ctx, desc, L, params, st, true, nullptr)) return rc;      // (also zeroes this step's dz maxima)
    const int head = L.n_sine;
    const bool z_head = hp_z_stash_ok(L.fan_in[head - 1]);
    if (int rc = hp_forward_pass(desc, L, params, fv, st, z_head)) return rc;
    return hp_head_forward(y, z_head ? reinterpret_cast<const char*>(fv.dact[head - 1]) : fv.act_hl(head),
                           params + L.w_off[head], params + L.b_off[head], n, desc->hidden_features, 0, 0.f, st, z_head,
                           layer_omega(desc, head - 1), fv.ctx.act_scale(head));
}

int inr_siren_backward_train(const inr_siren_desc_t* desc, const float* params, float* grads, const float* gy, int64_t n,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_desc(desc)) return rc;
    INR_REQUIRE(params && grads && gy, INR_E_INVALID, "inr_siren_backward_train: null pointer");
    INR_REQUIRE(n >= 1 && n <= MAX_ROWS, INR_E_INVALID, "inr_siren_backward_train: bad row count %lld", (long long)n);
    const Layout L = make_layout(desc);
    INR_REQUIRE(hp_eligible(desc, L), INR_E_INVALID, "inr_siren_backward_train: network shape not served by the pre-split kernels");
    INR_REQUIRE(aligned16(workspace) && aligned16(params) && aligned16(grads), INR_E_ALIGN,
                "inr_siren_backward_train: params/grads/workspace must be 16-byte aligned");
    const void* x = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_reuse_mu);
        ReuseStamp* s = reuse_find(workspace, false);
        INR_REQUIRE(s && s->fwd_train && s->n == n, INR_E_INVALID,
                    "inr_siren_backward_train: no inr_siren_forward_train of %lld rows is pending on this workspace", (long long)n);
        s->fwd_train = false;       // (the backward overwrites the stash with dz: one backward per forward)
        x = s->x;
    }
    const FitView fv = fit_view(desc, L, n, (const float*)x, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= fv.total, INR_E_WORKSPACE,
                "inr_siren_backward_train: workspace too small (%zu < %zu)", workspace_bytes, fv.total);
    hipStream_t st = (hipStream_t)stream;
    const int head = L.n_sine;
    const bool z_head = hp_z_stash_ok(L.fan_in[head - 1]);
    // the scale of the head's dz: max|gy| x max|w_head| x omega (measured: gy is the caller's)
    const HpSlots& s = fv.ctx.slots;
    if (int rc = h3_tensor_amax(s.gy_max(), gy, (long long)n * desc->out_features, st, 0u)) return rc;
    if (int rc = hp_head_bound_ext(s.head_bound(), s.gy_max(), params + L.w_off[head], desc->hidden_features,
                                   layer_omega(desc, head - 1), st))
        return rc;
    // "every element written" (include/inrhip.h): the finalize launch sums the tensors only, so the padding behind a tensor whose
    // length is no multiple of 4 floats -- the head's bias, at least -- is zeroed here
    for (int l = 0; l <= L.n_sine; ++l) {
        const long long w_end = L.w_off[l] + (long long)L.fan_in[l] * L.fan_out[l], b_end = L.b_off[l] + L.fan_out[l];
        const long long next = l < L.n_sine ? L.w_off[l + 1] : L.total;
        if (w_end < L.b_off[l]) INR_HIP(hipMemsetAsync(grads + w_end, 0, (size_t)(L.b_off[l] - w_end) * sizeof(float), st));
        if (b_end < next) INR_HIP(hipMemsetAsync(grads + b_end, 0, (size_t)(next - b_end) * sizeof(float), st));
    }
    FinalizeJob fin;
    float* loss_sink = fv.scratch + hp_slab_plan(L, n).loss_sink;
    if (int rc = hp_backward_pass(desc, L, params, grads, fv, nullptr, nullptr, gy, 1, loss_sink, st, fin, z_head)) return rc;
    return launch_finalize(fin, 0, 0.0, 0.0, 0.0, 0.0, st);
}

// ---- profiler --------------------------------------------------------------------------------------------
int inr_prof_enable(int enable) {
    g_prof.enabled = enable != 0;
    return 0;
}

int inr_prof_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (int k = 0; k < KC_COUNT; ++k) {
        for (auto& sp : g_prof.spans[k]) {
            g_prof.pool.push_back(sp.first);
            g_prof.pool.push_back(sp.second);
        }
        g_prof.spans[k].clear();
    }
    return 0;
}

int inr_prof_read(int kernel_class, int64_t* launches, double* total_ms) {
    INR_REQUIRE(kernel_class >= 0 && kernel_class < KC_COUNT && launches && total_ms, INR_E_INVALID,
                "inr_prof_read: bad arguments");
    std::lock_guard<std::mutex> lk(g_prof.mu);
    double ms = 0.0;
    for (auto& sp : g_prof.spans[kernel_class]) {
        INR_HIP(hipEventSynchronize(sp.second));
        float t = 0.f;
        INR_HIP(hipEventElapsedTime(&t, sp.first, sp.second));
        ms += t;
    }
    *launches = (int64_t)g_prof.spans[kernel_class].size();
    *total_ms = ms;
    return 0;
}

int inr_debug_set_ptr(int key, void* ptr) {
    if (key == 0) { g_stamps = (unsigned long long*)ptr; return 0; }
    if (key == 1) { g_h3_scratch = (char*)ptr; return 0; }
    return INR_E_INVALID;
}

// ---- diagnostic switches ------------------------------------------------------------------------------------------------
// One table: key -> switch, default, accepted range.  Process-global (see the header): every value is an atomic, so a switch can
// be read while another thread sets it, but a set is visible to every thread's next launch.
namespace {
struct DebugKey {
    int key;
    tune_int* var;
    int def, lo, hi;
};
tune_int g_rams_mode{2}, g_hybrid_mirror{1};   // (keys 14 and 2 fan out to other variables: kept here for inr_debug_get)
const DebugKey* debug_table(int* count) {
    static const DebugKey table[] = {
        {0, &g_force_generic, 0, 0, 1},   {1, &g_mfma16, 1, 0, 1},          {2, &g_hybrid_mirror, 1, 0, 1},
        {3, &g_h3, 1, 0, 2},              {5, &g_h3_serpentine, 1, 0, 1},   {6, &g_h3_wide, 1, 0, 1},
        {7, &g_hp, 1, 0, 1},              {8, &g_stamp_class, -1, -1, 3},   {9, &g_stamp_nth, 0, 0, 1 << 30},
        {10, &g_hp_persistent, 2, 0, 2},  {11, &g_hp_stagger, 0, 0, 1 << 20}, {12, &g_small_multi, 1, 0, 1},
        {13, &g_small_rows, 0, 0, 64},    {14, &g_rams_mode, 2, 0, 7},      {15, &g_rams_lds_waves, 42, 4, 42},
        {16, &g_hp_zhead, 1, 0, 1},       {17, &g_small_spin_limit, 0, 0, 1 << 30}, {18, &g_hp_narrow, 1, 0, 1},
        {19, &g_hp_fused_fwd, 0, 0, 1},  {20, &g_hp_side_stream, 1, 0, 1},  {21, &g_hp_head_min_rows, 16, 4, 256},
        {22, &g_hp_merge_blocks, 256, 28, 1024}, {23, &g_hp_head_rows, 0, 0, 4096},
        {24, &g_rams_epi_fuse, 2, 0, 2}, {25, &g_reduce_onepass, 1, 0, 1},
        {26, &g_rams_pregate_min_vox, 600000, 0, 1 << 30},
        {27, &g_hp_row, 0, 0, 1},        {28, &g_hp_row_min_tiles, 1024, 1, 1 << 30},
        {29, &g_hp_narrow_max_tiles, 192, 0, 1 << 30},
        {30, &g_hp_row_head, 1, 0, 1},   {31, &g_hp_row_head_min_tiles, 768, 1, 1 << 30},
        {32, &g_hp_grid_cap, 0, 0, 1 << 20},
    };
    *count = (int)(sizeof(table) / sizeof(table[0]));
    return table;
}
void debug_apply(const DebugKey& k, int value) {
    if (k.key == 14) {
        g_rams_h3 = value & 3;
        g_rams_force_lds = (value >> 2) & 1;
    } else if (k.key == 15) {
        value = (value == 8 || value == 16 || value == 42) ? value : 4;
    } else if (k.key == 2) {
        set_hybrid_variant(value);
    }
    k.var->store(value);
}
}  // namespace

int inr_debug_set(int key, int value) {
    int n = 0;
    const DebugKey* t = debug_table(&n);
    for (int i = 0; i < n; ++i)
        if (t[i].key == key) {
            INR_REQUIRE(value >= t[i].lo && value <= t[i].hi, INR_E_INVALID, "inr_debug_set: key %d takes %d .. %d (got %d)", key,
                        t[i].lo, t[i].hi, value);
            debug_apply(t[i], value);
            return 0;
        }
    INR_REQUIRE(false, INR_E_INVALID, "inr_debug_set: unknown key %d", key);
}

int inr_debug_get(int key, int* value) {
    INR_REQUIRE(value != nullptr, INR_E_INVALID, "inr_debug_get: null pointer");
    int n = 0;
    const DebugKey* t = debug_table(&n);
    for (int i = 0; i < n; ++i)
        if (t[i].key == key) {
            *value = t[i].var->load();
            return 0;
        }
    INR_REQUIRE(false, INR_E_INVALID, "inr_debug_get: unknown key %d", key);
}

int inr_debug_reset(void) {
    int n = 0;
    const DebugKey* t = debug_table(&n);
    for (int i = 0; i < n; ++i) debug_apply(t[i], t[i].def);
    g_stamps = nullptr;
    g_h3_scratch = nullptr;
    return 0;
}

int inr_launch_count(int family, int64_t* count) {
    const bool known = (family >= 0 && family < LF_COUNT) || (family >= INR_LF_ERD_BASE && family < INR_LF_ERD_END);
    INR_REQUIRE(known && count, INR_E_INVALID, "inr_launch_count: bad arguments");
    *count = (int64_t)g_launches[family].load(std::memory_order_relaxed);
    return 0;
}

int inr_pia_launch_count(int family, int64_t* count) {
    INR_REQUIRE(family >= 0 && family < INR_PIA_LF_COUNT && count, INR_E_INVALID, "inr_pia_launch_count: bad arguments");
    *count = (int64_t)g_launches[LF_PIA_BASE + family].load(std::memory_order_relaxed);
    return 0;
}

int inr_jet_launch_count(int family, int64_t* count) {
    INR_REQUIRE(family >= 0 && family < INR_JET_LF_COUNT && count, INR_E_INVALID, "inr_jet_launch_count: bad arguments");
    *count = (int64_t)g_launches[LF_JET_BASE + family].load(std::memory_order_relaxed);
    return 0;
}

int inr_launch_counts_reset(void) {
    for (auto& c : g_launches) c.store(0, std::memory_order_relaxed);
    return 0;
}

}  // extern "C"
