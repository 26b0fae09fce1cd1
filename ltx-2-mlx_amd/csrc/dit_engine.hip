// DiT engine: sequences the gfx950 kernels of one LTX-2 denoise step on a caller stream and owns
// the hipGraph of the distilled sampling loop.  Host-side only (no heavy kernels here).
//
// Restates the control flow of the reference's LTXModel.__call__ (LTX_2_MLX/model/transformer/
// model.py:776-881), BasicTransformerBlock.__call__ (transformer.py:191-238) and, for AudioVideo
// models, BasicAVTransformerBlock.__call__ (transformer.py:457-648) with
// MultiModalTransformerArgsPreprocessor (model.py:284-410).  Step-invariant work (caption
// projection, RoPE tables, and - when the text K/V are not sigma-modulated - the per-layer text
// cross-attention K/V) is hoisted into ltx2_dit_prepare*.
//
// A model is two "modalities" (video m[0], audio m[1]; audio absent for VideoOnly) that run the
// same per-block program (self-attention, text cross-attention, feed-forward) on their own widths,
// plus the audio<->video cross-modal attention between them.
//
// Every GEMM and attention is enqueued the same way: build the parameter block from the operands (gemm_dense_params / attn_params), add what
// the call needs through the named setters of gemm.h / attention.h, then hand it to dense() / attend().
#include <math.h>
#include <cmath>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ltx2hip.h"
#include "attention.h"
#include "fbc.h"
#include "gemm.h"
#include "rowops.h"
#include "sampler.h"

#define TRY(expr)                       \
    do {                                \
        int rc_ = (expr);               \
        if (rc_ != LTX2_OK) return rc_; \
    } while (0)

namespace {
struct Wt {
    const void* p;
    int dtype;
    long n;
};

struct AdaW {       // AdaLayerNormSingle (timestep_embedding.py:166-202)
    const bf16 *t1_w = nullptr, *t2_w = nullptr, *lin_w = nullptr;
    const float *t1_b = nullptr, *t2_b = nullptr, *lin_b = nullptr;
    int rows = 0;
};

struct AttnW {      // Attention (attention.py:144-253); self: fused qkv, cross: q + fused kv
    const bf16 *qkv_w = nullptr, *q_w = nullptr, *kv_w = nullptr, *o_w = nullptr, *g_w = nullptr;
    const float *qkv_b = nullptr, *q_b = nullptr, *kv_b = nullptr, *o_b = nullptr, *g_b = nullptr, *qn = nullptr,
                *kn = nullptr;
};

struct BlockW {     // one modality's share of a transformer block
    AttnW self, text;
    const bf16 *ff1_w = nullptr, *ff2_w = nullptr;
    const float *ff1_b = nullptr, *ff2_b = nullptr, *sst = nullptr, *prompt_sst = nullptr;
};

struct LayerW {
    BlockW m[2];
    AttnW a2v, v2a;
    const float* ca[2] = {nullptr, nullptr};     // scale_shift_table_a2v_ca_{video,audio}  [5][D]
};

struct ModW {       // per-modality model-level weights
    const bf16 *patch_w = nullptr, *cap1_w = nullptr, *cap2_w = nullptr, *proj_w = nullptr;
    const float *patch_b = nullptr, *cap1_b = nullptr, *cap2_b = nullptr, *proj_b = nullptr, *sst_out = nullptr;
    AdaW ada, prompt, cross_ss, cross_gate;
};

struct Mod {        // per-modality geometry + workspace
    int D = 0, H = 0, hd = 0, Cin = 0, Cout = 0;
    int N = 0, Npad = 0, S = 0, Spad = 0;
    float *x = nullptr, *sin_f = nullptr, *e1_f = nullptr, *e_f = nullptr, *emb = nullptr, *vel = nullptr, *x0 = nullptr,
          *cosb = nullptr, *sinb = nullptr, *ccos = nullptr, *csin = nullptr, *aux_e = nullptr, *prompt_emb = nullptr, *sst_all = nullptr, *comb = nullptr, *ca_all = nullptr, *ca_comb = nullptr,
          *cross_ss = nullptr, *cross_gate = nullptr, *glog = nullptr;
    int glog_parts = 1;                 // how the last gate_logits() call left m.glog: one array, or GATE_LOGIT_PARTS partial sums + glog_bias
    const float* glog_bias = nullptr;
    bf16 *lat = nullptr, *h = nullptr, *h2 = nullptr, *qkv = nullptr, *vt = nullptr, *att = nullptr, *ff = nullptr,
         *sin_b = nullptr, *e1_b = nullptr, *es_b = nullptr, *ctx_in = nullptr, *c1 = nullptr, *ctxp = nullptr,
         *ctxm = nullptr, *kv2 = nullptr, *vt2 = nullptr;
    const bf16* ctx = nullptr;      // projected text context (ctxp or ctx_in)
    unsigned long long* kmask = nullptr;   // text cross-attention key mask as 64-bit words (Modality.context_mask); used when has_kmask
    bool use_comb = false;             // this forward reads the combined AdaLN rows (comb) instead of (sst, emb)
    bool has_kmask = false;
    float* ts_tok = nullptr;        // per-token timesteps of a captured conditioned step: denoise_mask * sigma, formed on the device (per_token workspaces)
    float* qss = nullptr;           // text cross-attention with q_norm folded in: partial row sums of squares of the projected queries [N][D/64]
    float* knq = nullptr;           //   and k_norm.weight * q_norm.weight per layer [L][D] (the per-dim q weight moves onto the cached keys)
    bool qfold = false;             //   decided per prepare: the query projection runs on a kernel that writes the partial sums
    // round 6, the text cross-attention's pre-norm folded around the GEMMs (GemmParams::shadow / rf_parts; fold_supported()): h doubles as the bf16 shadow of the residual stream
    float* rss = nullptr;           //   partial sums of squares of the new residual rows, one per 256-column tile [D/256][rss_ld], left by attn1.to_out's epilogue
    long rss_ld = 0;                //   (the query projection turns them into its rows' RMS factors itself)
    int fold_max = 0;               //   what this geometry / model supports (prepare): 0 none, 1 the fold
    unsigned char* a8 = nullptr;    // fp8 compute: per-token e4m3fn codes of the current GEMM's activation operand [N][<= 4D]
    float* a8s = nullptr;           //              and their row scales [N]
};

inline long align_up(long v, long a = 256) { return (v + a - 1) / a * a; }
}  // namespace

struct ltx2_dit {
    ltx2_dit_config cfg{};
    bool av = false, v2 = false, gated = false;
    std::unordered_map<std::string, Wt> weights;
    std::vector<LayerW> layers;
    ModW mw[2];
    Mod m[2];
    bool resolved = false;
    char* ws = nullptr;
    long ws_bytes = 0;
    int per_token = 0;
    float* sigmas_dev = nullptr;       // 64 sigmas of a captured loop, then 64 sub-sigmas (the res_2s loop)
    float* r2s = nullptr;              // res_2s: x_mid | anchor | eps1, three fp32 workspaces allocated on first use, freed with the context
    long r2s_each = 0;                 //   elements of each: [N][Cout], on an AudioVideo context [N][Cout] and [Na][Cout_a] together
    float* heun = nullptr;             // Heun / GE: the video's prev | d | xp, then on an AudioVideo context the audio's d | xp; fp32, allocated on first use, freed with the context
    long heun_n = 0;                   //   elements in all: heun_total(c)
    bool heun_prev = false;            //   a step entry with GE and first != 0 has been enqueued since the workspace was allocated: prev holds a velocity
    double* pg_part = nullptr;         // projected guidance: the sums kernel's partials [pg_rows][5], allocated on first use for the bound N, freed with the context
    int pg_rows = 0;
    float* pg_run = nullptr;           //   and, for the legacy APG guider with momentum only, its running guidance [N][Cout] fp32
    long pg_run_n = 0;
    double* mm_part[2] = {};           // multi-modal guidance with rescale: each modality's partials [mm_rows[k]][4], allocated on first use for the bound shapes, freed with the context
    int mm_rows[2] = {};
    double* pgj_part[2] = {};          // joint projected guidance: each modality's partials [pgj_rows[k]][5], for the modalities whose guider reads sums; allocated on first use, freed with the context
    int pgj_rows[2] = {};
    double* cs_part = nullptr;         // CFG with the per-channel rescale: the statistics' partials [cs_rows][4][Cout], then the fp32 statistics [4][Cout] behind them (cs_stats);
    float* cs_stats = nullptr;         //   one allocation, made on first use for the bound shape, freed with the context
    int cs_rows = 0, cs_C = 0;
    float* xattn_gate = nullptr;       // ltx2_dit_set_cross_attn_scale: [D] fp32 holding the scale, the gate table of the text cross-attention's to_out in layers >= xattn_start;
    int xattn_start = 0;               //   allocated by the first scale != 1, freed with the context
    bool xattn_on = false;
    // fp8-resident linear weights: the typed `const bf16*` fields of the weight structs then hold the CODES pointer; dense() looks it
    // up here to hand the GEMM (codes, per-row scale) instead of bf16 weights.  Per context (a second context over the same tensors
    // -- the video twin of an AudioVideo model -- keeps its own entries); rebuilt whenever the weights are resolved again.
    std::unordered_map<const void*, const float*> fp8_scale;
    bool adaln_combine = true;         // ltx2_dit_set_option("adaln_combine"): round 4, see forward()
    bool text_kv_ahead = true;         // ltx2_dit_set_option("text_kv_ahead"): round 5, AudioVideo V2.3 -- the video stream's sigma-modulated text K / V of layer l are projected on the SIDE stream at the top of the layer
    hipEvent_t text_kv_ev = nullptr;   //   (they depend on the prompt and sigma only); the main stream waits on this event in front of its text cross-attention
    std::vector<unsigned char> stg[2]; // ltx2_dit_set_stg_blocks: per modality, the layers whose self-attention a PERTURBED forward leaves out (empty: none)
    int fold_norms = 1;                // ltx2_dit_set_option("fold_norms"): round 6, see block_attention(): 0 = every norm a pass of its own (round 5), 1 = the text cross-attention's
                                       //   plain RMS pre-norm rides on attn1.to_out's epilogue
    bool fp8_compute = false;          // ltx2_dit_set_option("fp8_compute"): fp8-resident weights x per-token fp8 activations on the fp8 MFMA
    bool prepared = false;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // AudioVideo: the audio modality's (small, latency-bound) kernels run on a side stream beside the video
    // GEMMs, whose 224-tile grids leave CUs idle; fork/join by events (captured as parallel graph branches).
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> sync_ev;
    size_t sync_next = 0;
    // live HIP-event profiling of one GEMM kernel instantiation (bench.py roofline)
    int prof_epi = -2;                 // -2 off, -1 every GEMM, >= 0 one epilogue
    std::vector<hipEvent_t> prof_ev;
    size_t prof_used = 0;
    double prof_flops = 0;
};

namespace {

// Carve the workspace; base == nullptr only computes the size.
long carve(ltx2_dit* c, char* base, int N, int S, int Na, int Sa, int per_token) {
    const long L = c->cfg.num_layers;
    long off = 0;
    auto take = [&](long bytes) {
        char* p = base ? base + off : nullptr;
        off += align_up(bytes);
        return p;
    };
    c->sigmas_dev = (float*)take(4L * 128);
    for (int k = 0; k < (c->av ? 2 : 1); ++k) {
        Mod& m = c->m[k];
        const long n = k ? Na : N, s = k ? Sa : S;
        const long D = m.D, npad = align_up(n, 64), spad = align_up(s, 64);
        const long Cctx = c->cfg.caption_channels > 0 ? c->cfg.caption_channels : D;
        const long T = per_token ? n : 1, rows = c->v2 ? 9 : 6;
        m.x = (float*)take(4L * n * D);
        m.lat = (bf16*)take(2L * n * m.Cin);
        m.h = (bf16*)take(2L * n * D);
        m.h2 = (bf16*)take(c->av ? 2L * n * D : 0);
        m.qkv = (bf16*)take(2L * n * 3 * D);      // also the cross-modal Q / K,V projected from this modality's tokens
        m.vt = (bf16*)take(2L * D * npad);
        m.att = (bf16*)take(2L * n * D);
        m.ff = (bf16*)take(2L * n * 4 * D);
        m.glog = (float*)take(c->gated ? 4L * n * m.H * GATE_LOGIT_PARTS : 0);       // (room for the K-slice partial sums of gate_logits_parts_launch)
        m.kmask = (unsigned long long*)take(8L * (spad / 64));
        m.qss = (float*)take(4L * n * (D / 64));
        m.knq = (float*)take(4L * L * D);
        const bool fold_bufs = k == 0 && !c->av;
        m.rss_ld = align_up(n, 256) + 256;
        m.rss = (float*)take(fold_bufs ? 4L * (D / 256 + 1) * m.rss_ld : 0);
        m.a8 = (unsigned char*)take((c->fp8_compute && k == 0) ? n * 4 * D : 0);
        m.a8s = (float*)take((c->fp8_compute && k == 0) ? 4L * n : 0);
        m.sin_f = (float*)take(4L * 256);
        m.e1_f = (float*)take(4L * D);
        m.aux_e = (float*)take(4L * D);
        m.e_f = (float*)take(4L * T * D);
        m.emb = (float*)take(4L * T * rows * D);
        m.prompt_emb = (float*)take(c->v2 ? 4L * 2 * D : 0);
        // round 4: every layer's scale_shift_table in one block (copied at prepare) and its per-step sum with the timestep embedding (adaln_combine)
        m.sst_all = (float*)take(4L * L * rows * D);
        m.comb = (float*)take(4L * L * rows * D);
        m.cross_ss = (float*)take(c->av ? 4L * 4 * D : 0);
        m.cross_gate = (float*)take(c->av ? 4L * D : 0);        // (directly behind cross_ss: the five cross-modal embedding rows are one block, see forward())
        m.ca_all = (float*)take(c->av ? 4L * L * 5 * D : 0);
        m.ca_comb = (float*)take(c->av ? 4L * L * 5 * D : 0);
        m.ts_tok = (float*)take(per_token ? 4L * n : 0);
        m.sin_b = (bf16*)take(per_token ? 2L * n * 256 : 0);
        m.e1_b = (bf16*)take(per_token ? 2L * n * D : 0);
        m.es_b = (bf16*)take(per_token ? 2L * n * D : 0);
        m.vel = (float*)take(4L * n * m.Cout);
        m.x0 = (float*)take(4L * n * m.Cout);
        m.cosb = (float*)take(4L * n * (D / 2));
        m.sinb = (float*)take(4L * n * (D / 2));
        const long Dc = c->m[c->av ? 1 : 0].D;         // cross-modal RoPE lives in the audio inner dim
        m.ccos = (float*)take(c->av ? 4L * n * (Dc / 2) : 0);
        m.csin = (float*)take(c->av ? 4L * n * (Dc / 2) : 0);
        m.ctx_in = (bf16*)take(2L * s * Cctx);
        m.c1 = (bf16*)take(c->cfg.caption_channels > 0 ? 2L * s * D : 0);
        m.ctxp = (bf16*)take(c->cfg.caption_channels > 0 ? 2L * s * D : 0);
        m.ctxm = (bf16*)take(c->v2 ? 2L * s * D : 0);
        const long kv_layers = c->v2 ? 1 : L;          // sigma-modulated text K/V cannot be cached per prompt
        m.kv2 = (bf16*)take(2L * kv_layers * s * 2 * D);
        m.vt2 = (bf16*)take(2L * kv_layers * D * spad);
    }
    return off;
}

const void* find(ltx2_dit* c, const std::string& name, int dtype, long numel) {
    auto it = c->weights.find(name);
    if (it == c->weights.end()) {
        ltx2_set_error("dit: missing weight '%s'", name.c_str());
        return nullptr;
    }
    if (dtype == LTX2_DTYPE_BF16 && it->second.dtype == LTX2_DTYPE_FP8_E4M3FN && it->second.n == numel) {
        auto sc = c->weights.find(name + "_scale");
        if (sc == c->weights.end() || sc->second.dtype != LTX2_DTYPE_F32) {
            ltx2_set_error("dit: fp8-resident weight '%s' has no fp32 '%s_scale' vector", name.c_str(), name.c_str());
            return nullptr;
        }
        c->fp8_scale[it->second.p] = (const float*)sc->second.p;
        return it->second.p;
    }
    if (it->second.dtype != dtype || it->second.n != numel) {
        ltx2_set_error("dit: weight '%s' has dtype %d / numel %ld, expected dtype %d / numel %ld", name.c_str(),
                       it->second.dtype, it->second.n, dtype, numel);
        return nullptr;
    }
    return it->second.p;
}

#define GETW(dst, name, rows, cols)                                                                          \
    do {                                                                                                     \
        dst = (const bf16*)find(c, std::string(name) + ".weight", LTX2_DTYPE_BF16, (long)(rows) * (cols));   \
        if (!dst) return LTX2_E_STATE;                                                                       \
    } while (0)
#define GETB(dst, name, n)                                                                    \
    do {                                                                                      \
        dst = (const float*)find(c, std::string(name) + ".bias", LTX2_DTYPE_F32, (long)(n));  \
        if (!dst) return LTX2_E_STATE;                                                        \
    } while (0)
#define GETF(dst, name, n)                                                          \
    do {                                                                            \
        dst = (const float*)find(c, std::string(name), LTX2_DTYPE_F32, (long)(n));  \
        if (!dst) return LTX2_E_STATE;                                              \
    } while (0)

int resolve_ada(ltx2_dit* c, AdaW& a, const std::string& name, long D, int rows) {
    GETW(a.t1_w, name + ".emb.timestep_embedder.linear_1", D, 256);
    GETB(a.t1_b, name + ".emb.timestep_embedder.linear_1", D);
    GETW(a.t2_w, name + ".emb.timestep_embedder.linear_2", D, D);
    GETB(a.t2_b, name + ".emb.timestep_embedder.linear_2", D);
    GETW(a.lin_w, name + ".linear", rows * D, D);
    GETB(a.lin_b, name + ".linear", rows * D);
    a.rows = rows;
    return LTX2_OK;
}

// query width Dq, key/value source width Dc, attention inner width Di, `heads` gate logits
int resolve_attn(ltx2_dit* c, AttnW& a, const std::string& name, long Dq, long Dc, long Di, int heads, bool self) {
    if (self) {
        GETW(a.qkv_w, name + ".to_qkv", 3 * Di, Dq);
        GETB(a.qkv_b, name + ".to_qkv", 3 * Di);
    } else {
        GETW(a.q_w, name + ".to_q", Di, Dq);
        GETB(a.q_b, name + ".to_q", Di);
        GETW(a.kv_w, name + ".to_kv", 2 * Di, Dc);
        GETB(a.kv_b, name + ".to_kv", 2 * Di);
    }
    GETW(a.o_w, name + ".to_out.0", Dq, Di);
    GETB(a.o_b, name + ".to_out.0", Dq);
    GETF(a.qn, name + ".q_norm.weight", Di);
    GETF(a.kn, name + ".k_norm.weight", Di);
    if (c->gated) {
        GETW(a.g_w, name + ".to_gate_logits", heads, Dq);
        GETB(a.g_b, name + ".to_gate_logits", heads);
    }
    return LTX2_OK;
}

int resolve(ltx2_dit* c) {
    if (c->resolved) return LTX2_OK;
    c->fp8_scale.clear();
    const int nm = c->av ? 2 : 1;
    const int rows = c->v2 ? 9 : 6;
    for (int k = 0; k < nm; ++k) {
        const std::string pre = k ? "audio_" : "";
        const long D = c->m[k].D;
        ModW& w = c->mw[k];
        GETW(w.patch_w, pre + "patchify_proj", D, c->m[k].Cin);
        GETB(w.patch_b, pre + "patchify_proj", D);
        TRY(resolve_ada(c, w.ada, pre + "adaln_single", D, rows));
        if (c->v2) TRY(resolve_ada(c, w.prompt, pre + "prompt_adaln_single", D, 2));
        if (c->cfg.caption_channels > 0) {
            GETW(w.cap1_w, pre + "caption_projection.linear_1", D, c->cfg.caption_channels);
            GETB(w.cap1_b, pre + "caption_projection.linear_1", D);
            GETW(w.cap2_w, pre + "caption_projection.linear_2", D, D);
            GETB(w.cap2_b, pre + "caption_projection.linear_2", D);
        }
        GETF(w.sst_out, pre + "scale_shift_table", 2 * D);
        GETW(w.proj_w, pre + "proj_out", c->m[k].Cout, D);
        GETB(w.proj_b, pre + "proj_out", c->m[k].Cout);
    }
    if (c->av) {
        TRY(resolve_ada(c, c->mw[0].cross_ss, "av_ca_video_scale_shift_adaln_single", c->m[0].D, 4));
        TRY(resolve_ada(c, c->mw[0].cross_gate, "av_ca_a2v_gate_adaln_single", c->m[0].D, 1));
        TRY(resolve_ada(c, c->mw[1].cross_ss, "av_ca_audio_scale_shift_adaln_single", c->m[1].D, 4));
        TRY(resolve_ada(c, c->mw[1].cross_gate, "av_ca_v2a_gate_adaln_single", c->m[1].D, 1));
    }
    c->layers.assign(c->cfg.num_layers, LayerW());
    for (int i = 0; i < c->cfg.num_layers; ++i) {
        LayerW& w = c->layers[i];
        const std::string p = "transformer_blocks." + std::to_string(i) + ".";
        for (int k = 0; k < nm; ++k) {
            const std::string pre = k ? "audio_" : "";
            const long D = c->m[k].D;
            BlockW& b = w.m[k];
            TRY(resolve_attn(c, b.self, p + pre + "attn1", D, D, D, c->m[k].H, true));
            TRY(resolve_attn(c, b.text, p + pre + "attn2", D, D, D, c->m[k].H, false));
            GETW(b.ff1_w, p + pre + "ff.net.0.proj", 4 * D, D);
            GETB(b.ff1_b, p + pre + "ff.net.0.proj", 4 * D);
            GETW(b.ff2_w, p + pre + "ff.net.2", D, 4 * D);
            GETB(b.ff2_b, p + pre + "ff.net.2", D);
            GETF(b.sst, p + pre + "scale_shift_table", rows * D);
            if (c->v2) GETF(b.prompt_sst, p + pre + "prompt_scale_shift_table", 2 * D);
        }
        if (c->av) {
            const long Dv = c->m[0].D, Da = c->m[1].D;
            TRY(resolve_attn(c, w.a2v, p + "audio_to_video_attn", Dv, Da, Da, c->m[1].H, false));
            TRY(resolve_attn(c, w.v2a, p + "video_to_audio_attn", Da, Dv, Da, c->m[1].H, false));
            GETF(w.ca[0], p + "scale_shift_table_a2v_ca_video", 5 * Dv);
            GETF(w.ca[1], p + "scale_shift_table_a2v_ca_audio", 5 * Da);
        }
    }
    c->resolved = true;
    return LTX2_OK;
}
#undef GETW
#undef GETB
#undef GETF

thread_local ltx2_dit* g_prof_ctx = nullptr;

// fp8-resident weight: p.W then holds the codes pointer; hand the GEMM (codes, per-row scale) instead, expanded inside the kernel.  false: dense 16-bit weights
bool resident_fp8(ltx2_dit* c, GemmParams& p) {
    auto f8 = c->fp8_scale.find((const void*)p.W);
    if (f8 == c->fp8_scale.end()) return false;
    gemm_set_w8(p, p.W, f8->second);
    return true;
}

// fp8 compute (opt-in): would dense() send this GEMM to the fp8 MFMA?  (the video stream's big GEMMs on fp8-resident weights)
bool f8_route(ltx2_dit* c, const bf16* W, int M, int N, int K, int epi) {
    if (!c->fp8_compute || !c->m[0].a8 || M < 1024 || M > c->m[0].N || K > 4 * c->m[0].D) return false;
    GemmParams q = gemm_dense_params(nullptr, K, W, nullptr, c->m[0].x, 8, M, N, K);
    if (!resident_fp8(c, q)) return false;
    gemm_set_a8(q, c->m[0].a8, c->m[0].a8s, K);
    return gemm_v4_f8_supported(q, epi);
}

// q_norm folded into the text cross-attention (round 3, VERDICT r2 #4c): possible when the query projection runs on a kernel whose
// epilogue writes the row partial sums of squares (the 4-wave kernel's bf16 epilogue: M >= 1024; D % 1024 == 0: the attention kernel's four lanes of a
// query row read the D / 64 partials as f32x4 quarters, so q_ss_ld = D / 64 must be a multiple of 16 -- ADVICE r5: D = 512 / 1536 / 2560 / 3584 fall back to the unfused q_norm pass)
bool text_qfold_ok(ltx2_dit* c, int k) {
    const Mod& m = c->m[k];
    if (m.D % 1024 != 0 || m.hd != 128) return false;
    const bf16* W = c->layers[0].m[k].text.q_w;
    GemmParams q = gemm_dense_params(m.h, m.D, W, nullptr, m.x, m.D, m.N, m.D, m.D);
    resident_fp8(c, q);
    if (k == 0 && f8_route(c, W, m.N, m.D, m.D, EPI_BF16)) gemm_set_a8(q, m.a8, m.a8s, m.D);
    return gemm_rowss_supported(q, EPI_BF16);
}

// round 6: can the text cross-attention's pre-norm of this modality's blocks be folded around attn1.to_out / attn2.to_q (block_attention())?  VideoOnly non-V2.3
// ungated models on dense bf16 weights in the bfloat16 build (the un-normalised shadow is not safe in IEEE half: gemm_fold_supported() refuses the float16 build),
// both GEMMs on the 4-wave layout-3 kernel
int fold_supported(ltx2_dit* c, int k) {
    if (c->av || c->v2 || c->gated || c->fp8_compute || !c->fp8_scale.empty() || k != 0) return 0;
    const Mod& m = c->m[k];
    if (!m.rss || m.D % 256 != 0 || m.D / 256 > GEMM_RF_MAX_PARTS) return 0;
    const BlockW& w = c->layers[0].m[k];
    // producer: attn1.to_out; consumer: attn2.to_q
    GemmParams q = gemm_dense_params(m.h, m.D, w.self.o_w, nullptr, m.x, m.D, m.N, m.D, m.D);
    gemm_set_fold_producer(q, m.h, m.D, nullptr, m.rss, m.rss_ld);
    if (!gemm_fold_supported(q, EPI_RESID_GATE_F32)) return 0;
    GemmParams r = gemm_dense_params(m.h, m.D, w.text.q_w, nullptr, m.qkv, m.D, m.N, m.D, m.D);
    gemm_set_fold_consumer(r, m.rss, m.rss_ld, m.D / 256, m.D, c->cfg.norm_eps);
    if (!gemm_fold_supported(r, EPI_BF16)) return 0;
    return 1;
}

__global__ void vec_mul_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] * b[i];
}

// One GEMM of the engine.  The caller builds p (gemm_dense_params, then gemm_set_gate / gemm_set_vt / gemm_set_fold_* / p.rowss as the call needs); dense()
// adds what only the engine knows: fp8-resident weights, the fp8-compute route, whether the epilogue can write a requested V^T, and the profiling bracket.
// preq: the kernel that produced A already left its per-token e4m3fn codes + scales in m[0].a8 / a8s (norm_mod_launch's q8 output);
// only valid when f8_route() says yes for this GEMM
// vt_done (with gemm_set_vt): whether the GEMM's epilogue wrote V^T (else the caller runs vt_transpose_launch on the V columns of `out`)
int dense(ltx2_dit* c, GemmParams p, int epi, hipStream_t st, bool preq = false, bool* vt_done = nullptr) {
    const bf16* const A = p.A;
    const bf16* const W = p.W;
    if (!c->fp8_scale.empty()) resident_fp8(c, p);
    // fp8 compute (opt-in): the video stream's big GEMMs on fp8-resident weights take per-token-quantised activations and the fp8 MFMA
    if (p.W8 && f8_route(c, W, p.M, p.N, p.K, epi)) {
        if (!preq) TRY(quant_rows_fp8_launch(A, p.lda, p.M, p.K, c->m[0].a8, p.K, c->m[0].a8s, st));
        gemm_set_a8(p, c->m[0].a8, c->m[0].a8s, p.K);
    } else if (preq) {
        ltx2_set_error("dit: a pre-quantised activation reached a GEMM that does not take the fp8 path");
        return LTX2_E_STATE;
    }
    if (p.vt) {
        *vt_done = gemm_vt_fused(p, epi);
        if (!*vt_done) p.vt = nullptr;
    }
    ltx2_dit* pc = g_prof_ctx;
    const bool prof = pc && (pc->prof_epi == -1 || pc->prof_epi == epi);
    if (prof) {
        while (pc->prof_ev.size() < pc->prof_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return LTX2_E_HIP;
            pc->prof_ev.push_back(e);
        }
        (void)hipEventRecord(pc->prof_ev[pc->prof_used], st);
    }
    const int rc = gemm_launch(p, epi, false, st);
    if (prof) {
        (void)hipEventRecord(pc->prof_ev[pc->prof_used + 1], st);
        pc->prof_used += 2;
        pc->prof_flops += 2.0 * p.M * p.N * p.K;
    }
    return rc;
}

// timesteps of a conditioned step (reference pipelines/common.py:193-232 timesteps_from_mask): ts[n] = mask[n] * sigma, sigma read on the device
__global__ void mask_sigma_kernel(const float* __restrict__ mask, const float* __restrict__ sigma, float* __restrict__ ts, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ts[i] = mask[i] * sigma[0];
}

__global__ void silu_cast_kernel(const float* __restrict__ in, bf16* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = f2bf(silu_f(in[i]));
}

// AdaLayerNormSingle over T rows of timesteps (ts[i*t_stride] * mult): emb [T][rows*D] (fp32) and,
// when e_out != null, the embedded timestep e [T][D] (model.py:113-140).
int adaln_chain(ltx2_dit* c, Mod& m, const AdaW& a, const float* ts, long t_stride, int T, float mult, float* emb, float* e_out,
                hipStream_t st) {
    const int D = m.D;
    if (T == 1) {
        float* e = e_out ? e_out : m.aux_e;
        TRY(timestep_sinusoid_launch(ts, 0, 0.f, mult, 1, 256, m.sin_f, nullptr, st));
        TRY(gemv_launch(m.sin_f, 256, a.t1_w, a.t1_b, m.e1_f, D, 1, D, 256, 0, 1, st));
        TRY(gemv_launch(m.e1_f, D, a.t2_w, a.t2_b, e, D, 1, D, D, 0, 0, st));
        TRY(gemv_launch(e, D, a.lin_w, a.lin_b, emb, (long)a.rows * D, 1, a.rows * D, D, 1, 0, st));
    } else {
        TRY(timestep_sinusoid_launch(ts, t_stride, 0.f, mult, T, 256, nullptr, m.sin_b, st));
        TRY(dense(c, gemm_dense_params(m.sin_b, 256, a.t1_w, a.t1_b, m.e1_b, D, T, D, 256), EPI_SILU_BF16, st));
        TRY(dense(c, gemm_dense_params(m.e1_b, D, a.t2_w, a.t2_b, e_out, D, T, D, D), EPI_F32, st));
        hipLaunchKernelGGL(silu_cast_kernel, dim3(2048), dim3(256), 0, st, e_out, m.es_b, (long)T * D);
        LTX2_CHECK_LAUNCH("silu_cast_kernel");
        TRY(dense(c, gemm_dense_params(m.es_b, D, a.lin_w, a.lin_b, emb, (long)a.rows * D, T, a.rows * D, D), EPI_F32, st));
    }
    return LTX2_OK;
}

// per-head gate logits as gate_logits() left them: one [rows][H] array, or GATE_LOGIT_PARTS partial sums + the bias (summed in the attention kernel's epilogue)
struct GateRef {
    const float* p = nullptr;
    int parts = 1;
    const float* bias = nullptr;
};
// the engine's softmax scale (1 / sqrt(d)) * log2(e), as attn_params() takes it
inline float scale_log2e(int hd) { return 1.4426950408889634f / sqrtf((float)hd); }
// One attention of the engine: a from attn_params() (+ attn_set_rowscale / a.kmask); gate = glog(): per-head gate logits [Nq][H] (V2.3), out *= 2 sigmoid(.) in the kernel's epilogue
int attend(AttnParams a, GateRef gate, hipStream_t st) {
    attn_set_gate(a, gate.p, a.H, gate.parts, gate.bias);
    return attn_launch(a, st);
}

// One event per fork/join edge of a forward (or of a whole captured loop): the pool grows on demand and
// is rewound at the start of every eager call / capture, so no event is re-recorded inside a capture.
hipEvent_t next_event(ltx2_dit* c) {
    if (c->sync_next == c->sync_ev.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        c->sync_ev.push_back(e);
    }
    return c->sync_ev[c->sync_next++];
}

// `to` continues after everything enqueued on `from` so far
int stream_after(ltx2_dit* c, hipStream_t from, hipStream_t to) {
    if (from == to) return LTX2_OK;
    hipEvent_t e = next_event(c);
    if (!e || hipEventRecord(e, from) != hipSuccess || hipStreamWaitEvent(to, e, 0) != hipSuccess) {
        ltx2_set_error("dit: stream fork/join failed: %s", hipGetErrorString(hipGetLastError()));
        return LTX2_E_HIP;
    }
    return LTX2_OK;
}

// split form of stream_after: record now (the point on `from` others may wait for), make `to` wait later
hipEvent_t event_record(ltx2_dit* c, hipStream_t from) {
    hipEvent_t e = next_event(c);
    if (!e || hipEventRecord(e, from) != hipSuccess) {
        ltx2_set_error("dit: event record failed: %s", hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    return e;
}

int event_wait(hipEvent_t e, hipStream_t to) {
    if (!e || hipStreamWaitEvent(to, e, 0) != hipSuccess) {
        ltx2_set_error("dit: stream wait failed: %s", hipGetErrorString(hipGetLastError()));
        return LTX2_E_HIP;
    }
    return LTX2_OK;
}

// Per-head gates (attention.py:241-249): att[:, h*hd:(h+1)*hd] *= 2*sigmoid(x @ Wg^T + bg)[:, h]
// many rows: K-slice partial sums, added (with the bias) by the attention kernel's epilogue; few rows (the audio stream): the one-launch form
inline bool gate_in_parts(int rows, int Dq) { return rows >= 1024 && Dq % (GATE_LOGIT_PARTS * 32) == 0 && Dq <= 8192; }
int gate_logits(ltx2_dit* c, Mod& m, const AttnW& w, const bf16* xin, int Dq, int rows, int H, hipStream_t st) {
    if (!c->gated) return LTX2_OK;
    m.glog_parts = gate_in_parts(rows, Dq) ? GATE_LOGIT_PARTS : 1;
    m.glog_bias = w.g_b;
    if (m.glog_parts > 1) return gate_logits_parts_launch(xin, Dq, w.g_w, m.glog, rows, Dq, H, st);
    return gate_logits_launch(xin, Dq, w.g_w, w.g_b, m.glog, H, rows, Dq, H, st);
}

// the gate logits gate_logits() left for the attention that follows (null for ungated models): the kernel's epilogue applies 2 sigmoid(.) per head
GateRef glog(ltx2_dit* c, const Mod& m) { return c->gated ? GateRef{m.glog, m.glog_parts, m.glog_bias} : GateRef{}; }

// K (k_norm applied, optional RoPE) and V^T of a text / cross-modal context.  p: the fused K | V projection (N = 2 Di, heads of hd); kn: the K half's norm weight
int project_kv(ltx2_dit* c, GemmParams p, bf16* vt, int npad, int hd, const float* kn, const float* cosb, const float* sinb, hipStream_t st) {
    const int Di = p.N / 2;
    bf16* const kv = (bf16*)p.out;
    gemm_set_vt(p, vt, Di, npad, hd);
    bool vt_done = false;           // V^T straight from the K/V GEMM's epilogue where the 4-wave kernel takes the shape
    TRY(dense(c, p, EPI_BF16, st, /*preq=*/false, &vt_done));
    const int offs[1] = {0};
    const float* wts[1] = {kn};
    TRY(qknorm_rope_launch(kv, 2 * Di, p.M, Di, hd, 1, offs, wts, c->cfg.norm_eps, cosb, sinb, st));
    if (vt_done) return LTX2_OK;
    return vt_transpose_launch(kv + Di, 2 * Di, vt, p.M, npad, Di / hd, st, hd);
}

// V2.3: the prompt-AdaLN-modulated text context of layer l and its K / V^T (transformer.py:427-455) -- a function of the prompt and sigma only
int text_kv(ltx2_dit* c, int k, int l, hipStream_t st) {
    Mod& m = c->m[k];
    const BlockW& w = c->layers[l].m[k];
    const int D = m.D;
    TRY(ctx_mod_launch(m.ctx, m.ctxm, m.S, D, w.prompt_sst + D, w.prompt_sst, m.prompt_emb + D, m.prompt_emb, st));
    return project_kv(c, gemm_dense_params(m.ctxm, D, w.text.kv_w, w.text.kv_b, m.kv2, 2 * D, m.S, 2 * D, D), m.vt2, m.Spad, m.hd,
                      m.qfold ? m.knq + (long)l * D : w.text.kn, nullptr, nullptr, st);
}

// ---- round 6: the text cross-attention's plain RMS pre-norm folded around the two GEMMs beside it ----------------------------------------------------
// rms_norm(x) in front of attn2.to_q (W, b) equals r (x W^T) + b with the row factor r = rsqrt(mean x^2 + eps).  attn1.to_out's gated-residual epilogue, which
// forms x, also leaves y = bf16(x) in `h` with the partial sums of squares of x (GemmParams::shadow), and the query projection takes (y, the partial sums -> r
// inside the kernel): the norm pass between the two GEMMs (15 us, 85 MB) is gone.  Same mathematics, another rounding order: y is rounded before the row factor
// instead of after it (both relative 2^-9).  Row-invariant gates only (one timestep per modality).
// The same algebra covers the two AdaLN-modulated norms (self-attention, feed-forward): the scale rides on the shadow, and the shift's product t W^T can be formed
// one step ahead by the projection itself from an extra operand row.  That was built and measured in this round (git history: "fold: its own kernel
// instantiations"): every kernel-level figure favoured it (three norm passes, 52 us per layer, for ~20 us of epilogue work), the step did not -- +0.3 ... +0.5 ms:
// the GEMMs on both sides run 4-5 % slower inside the step than their stand-alone A/B says (profiles/r06_fold_norms.md).  Only this one stayed.

// AdaLN rows of layer l: table row r + embedding row r; with one timestep per modality the sum was formed for every layer at the top of forward()
// (tab = the sums, no embedding rows)
struct AdaRows {
    const float* tab;
    const float* emb0;
    int D;
    const float* E(int r) const { return emb0 ? emb0 + (long)r * D : nullptr; }
};
AdaRows ada_rows(const ltx2_dit* c, const Mod& m, const BlockW& w, int l) {
    return {m.use_comb ? m.comb + (long)l * (c->v2 ? 9 : 6) * m.D : w.sst, m.use_comb ? nullptr : m.emb, m.D};
}

// Self-attention, text cross-attention of one modality (transformer.py:503-554 / 191-226)
// skip_self (a perturbed forward, STG; transformer.py:485-515): the self-attention sub-block is launches that do not happen -- the residual stream is
// unchanged, so its norm, gate logits, QKV projection, QK-norm + RoPE, V^T, attention and out-projection are all left out.  Its out-projection is also
// the fold's producer: such a layer runs its text cross-attention unfolded.  Only kernels are skipped, never an event record or wait.
int block_attention(ltx2_dit* c, int k, int l, long es, hipStream_t st, int fold = 0, bool skip_self = false) {
    Mod& m = c->m[k];
    const BlockW& w = c->layers[l].m[k];
    const int N = m.N, D = m.D, H = m.H, hd = m.hd;
    const float eps = c->cfg.norm_eps;
    const AdaRows ada = ada_rows(c, m, w, l);
    const float* const tab = ada.tab;
    // self-attention: AdaLN rows (shift, scale, gate) = sst[0:3] + emb[0:3]
    // fp8 compute: the norm kernels hand the following GEMM per-token e4m3fn codes directly (and skip the bf16 copy nobody else reads)
    const bool q1 = k == 0 && f8_route(c, w.self.qkv_w, N, 3 * D, D, EPI_BF16);
    const int fl = (k == 0 && !skip_self) ? fold : 0;
    if (!skip_self) {
        TRY(norm_mod_launch(m.x, D, (q1 && !c->gated) ? nullptr : m.h, D, N, D, eps, 0, tab + D, tab, ada.E(1), ada.E(0), es, st, q1 ? m.a8 : nullptr, D,
                            q1 ? m.a8s : nullptr));
        TRY(gate_logits(c, m, w.self, m.h, D, N, H, st));
        bool vt_done = false;           // the QKV GEMM's epilogue writes V^T itself where it can (gemm_v4.hip)
        {
            GemmParams p = gemm_dense_params(m.h, D, w.self.qkv_w, w.self.qkv_b, m.qkv, 3 * D, N, 3 * D, D);
            gemm_set_vt(p, m.vt, 2 * D, m.Npad, hd);
            TRY(dense(c, p, EPI_BF16, st, q1, &vt_done));
        }
        {
            const int offs[2] = {0, D};
            const float* wts[2] = {w.self.qn, w.self.kn};
            TRY(qknorm_rope_launch(m.qkv, 3 * D, N, D, hd, 2, offs, wts, eps, m.cosb, m.sinb, st));
        }
        if (!vt_done) TRY(vt_transpose_launch(m.qkv + 2 * D, 3 * D, m.vt, N, m.Npad, H, st, hd));
        TRY(attend(attn_params(m.qkv, 3 * D, m.qkv + D, 3 * D, m.vt, m.Npad, m.att, D, N, N, H, hd, scale_log2e(hd)), glog(c, m), st));
        GemmParams p = gemm_dense_params(m.att, D, w.self.o_w, w.self.o_b, m.x, D, N, D, D);
        gemm_set_gate(p, ada.E(2), es, tab + 2 * D);
        // the new residual rows also leave as the cross-attention query projection's operand (plain RMS norm: no scale, no shift): their shadow into h, its partial sums into rss
        if (fl >= 1) gemm_set_fold_producer(p, m.h, D, nullptr, m.rss, m.rss_ld);
        TRY(dense(c, p, EPI_RESID_GATE_F32, st));
    }

    // text cross-attention: no RoPE, no mask.  V1: plain RMSNorm on x, K/V cached per prompt.
    // V2.3 (transformer.py:427-455): q side modulated by rows (6,7) and gated by row 8; the context
    // is modulated by the prompt AdaLN (rows shift, scale), so K/V are recomputed every step.
    const bf16* kk;
    const bf16* vt;
    const bool q2 = k == 0 && f8_route(c, w.text.q_w, N, D, D, EPI_BF16);
    bf16* h2 = (q2 && !c->gated) ? nullptr : m.h;
    unsigned char* a8q = q2 ? m.a8 : nullptr;
    float* a8sq = q2 ? m.a8s : nullptr;
    if (c->v2) {
        TRY(norm_mod_launch(m.x, D, h2, D, N, D, eps, 0, tab + 7 * D, tab + 6 * D, ada.E(7), ada.E(6), es, st, a8q, D, a8sq));
        if (k == 0 && c->text_kv_ev) {      // projected ahead on the side stream (forward()): wait for it here
            TRY(event_wait(c->text_kv_ev, st));
            c->text_kv_ev = nullptr;
        } else {
            TRY(text_kv(c, k, l, st));
        }
        kk = m.kv2;
        vt = m.vt2;
    } else {
        if (fl < 1) TRY(norm_mod_launch(m.x, D, h2, D, N, D, eps, 0, nullptr, nullptr, nullptr, nullptr, 0, st, a8q, D, a8sq));
        kk = m.kv2 + (long)l * m.S * 2 * D;
        vt = m.vt2 + (long)l * D * m.Spad;
    }
    TRY(gate_logits(c, m, w.text, m.h, D, N, H, st));
    // q_norm folded (m.qfold): the projection's epilogue leaves the partial sums of squares of its rows; q_norm.weight already sits on the keys
    // (k_norm.weight * q_norm.weight, prepare) and the row's RMS factor becomes its softmax scale -- no pass over q between GEMM and attention
    {
        GemmParams p = gemm_dense_params(m.h, D, w.text.q_w, w.text.q_b, m.qkv, D, N, D, D);
        if (m.qfold) p.rowss = m.qss;
        if (fl >= 1) gemm_set_fold_consumer(p, m.rss, m.rss_ld, D / 256, D, eps);          // h holds the shadow: the row factors come from rss
        TRY(dense(c, p, EPI_BF16, st, q2));
    }
    if (!m.qfold) {
        const int offs[1] = {0};
        const float* wts[1] = {w.text.qn};
        TRY(qknorm_rope_launch(m.qkv, D, N, D, hd, 1, offs, wts, eps, nullptr, nullptr, st));
    }
    {
        AttnParams a = attn_params(m.qkv, D, kk, 2 * D, vt, m.Spad, m.att, D, N, m.S, H, hd, scale_log2e(hd));
        if (m.qfold) attn_set_rowscale(a, m.qss, D / 64, D, eps);          // q_norm as a per-row softmax scale from the projection's partial sums
        if (m.has_kmask) a.kmask = m.kmask;
        TRY(attend(a, glog(c, m), st));
    }
    GemmParams po = gemm_dense_params(m.att, D, w.text.o_w, w.text.o_b, m.x, D, N, D, D);
    if (c->v2) gemm_set_gate(po, ada.E(8), es, tab + 8 * D);
    else if (c->xattn_on && l >= c->xattn_start) gemm_set_gate(po, nullptr, 0, c->xattn_gate);      // cross_attn_scale: a row-invariant gate table
    return dense(c, po, EPI_RESID_GATE_F32, st);
}

// Feed-forward: AdaLN rows 3..5 (transformer.py:229-236,622-642); Linear -> GELU(tanh) -> Linear
int block_ffn(ltx2_dit* c, int k, int l, long es, hipStream_t st) {
    Mod& m = c->m[k];
    const BlockW& w = c->layers[l].m[k];
    const int N = m.N, D = m.D;
    const AdaRows ada = ada_rows(c, m, w, l);
    const float* const tab = ada.tab;
    const bool q3 = k == 0 && f8_route(c, w.ff1_w, N, 4 * D, D, EPI_GELU_BF16);
    TRY(norm_mod_launch(m.x, D, q3 ? nullptr : m.h, D, N, D, c->cfg.norm_eps, 0, tab + 4 * D, tab + 3 * D, ada.E(4), ada.E(3), es, st,
                        q3 ? m.a8 : nullptr, D, q3 ? m.a8s : nullptr));
    TRY(dense(c, gemm_dense_params(m.h, D, w.ff1_w, w.ff1_b, m.ff, 4 * D, N, 4 * D, D), EPI_GELU_BF16, st, q3));
    GemmParams p2 = gemm_dense_params(m.ff, 4 * D, w.ff2_w, w.ff2_b, m.x, D, N, D, 4 * D);
    gemm_set_gate(p2, ada.E(5), es, tab + 5 * D);
    return dense(c, p2, EPI_RESID_GATE_F32, st);
}

// Audio <-> video cross-modal attention (transformer.py:556-620).  Table rows
// (scale_a2v, shift_a2v, scale_v2a, shift_v2a, gate); both directions read the SAME pre-update
// RMS-normalised streams, so all four modulated inputs are formed before x is touched.
//
// Round 4 schedule (was: 23 kernels in one chain on the main stream, ~500 us per layer with the chip mostly idle).  Only the audio -> video
// direction feeds the video stream (its feed-forward reads the a2v update); the video -> audio direction updates the AUDIO stream only.  So:
//   main (video): ONE norm launch for both modulations of vx -> a2v query projection -> rope(q) -> [audio K/V ready] -> a2v attention ->
//                 out-projection into vx -> (caller) video feed-forward
//   side (audio): ONE norm launch for both modulations of ax -> a2v K/V from audio (skinny) -> [signal] -> v2a query (skinny) -> [vx modulations
//                 ready] -> v2a key / value projection (the other big video-side GEMM) -> k-norm + rope -> v2a attention -> out-projection into ax ->
//                 (caller) audio feed-forward
// Buffers: the video modality's qkv scratch holds the a2v queries [N][Da] and, behind them, the v2a keys / values [N][2 Da]; the audio modality's
// holds the a2v keys / values [Na][2 Da] and, behind them, the v2a queries [Na][Da] -- the two directions never share a region.
int block_cross_modal(ltx2_dit* c, int l, hipStream_t st, hipStream_t sa) {
    Mod &v = c->m[0], &a = c->m[1];
    const LayerW& w = c->layers[l];
    const int Dv = v.D, Da = a.D, H = a.H, hd = a.hd;
    const float eps = c->cfg.norm_eps;
    const bool comb = c->adaln_combine;          // table + embedding rows already summed for every layer (forward())
    const float *tv = comb ? v.ca_comb + (long)l * 5 * Dv : w.ca[0], *ta = comb ? a.ca_comb + (long)l * 5 * Da : w.ca[1];
    const int offs[1] = {0};
    bf16* v_q = v.qkv;                              // a2v queries  [N][Da]
    bf16* v_kv = v.qkv + (long)v.N * Da;            // v2a keys | values [N][2 Da]
    bf16* a_kv = a.qkv;                             // a2v keys | values [Na][2 Da]
    bf16* a_q = a.qkv + (long)a.N * 2 * Da;         // v2a queries [Na][Da]
    // Capture order matters under hipGraph: a node's FIRST captured child continues its stream's run list (ROCm executes a run list serially), so
    // after every event record the recording stream's own next kernel is enqueued before the other stream's wait + consumer.
    // ---- video side, main stream: both modulations of vx, the two video-side projections ----
    {
        const float* sct[2] = {tv, tv + 2 * Dv};
        const float* sht[2] = {tv + Dv, tv + 3 * Dv};
        const float* sce[2] = {comb ? nullptr : v.cross_ss, comb ? nullptr : v.cross_ss + 2 * Dv};
        const float* she[2] = {comb ? nullptr : v.cross_ss + Dv, comb ? nullptr : v.cross_ss + 3 * Dv};
        TRY(norm_mod2_launch(v.x, Dv, v.h, v.h2, Dv, v.N, Dv, eps, sct, sht, sce, she, st));       // a2v query side | v2a context side
    }
    // the v2a key / value projection (the other big video-side GEMM) runs on the side stream from here, beside the main stream's a2v chain: same-box
    // A/B of the LTX-2.3 step, hipGraph: 104.0 ms against 106.0 with both projections in ONE launch on the main stream (128 + 256 tiles are two rounds
    // of the 256 CUs whichever way they are launched; on two streams the second round overlaps the a2v chain's small kernels)
    bool vt_done = false;
    hipEvent_t video_norm = event_record(c, st);
    if (!video_norm) return LTX2_E_HIP;
    TRY(gate_logits(c, v, w.a2v, v.h, Dv, v.N, H, st));
    TRY(dense(c, gemm_dense_params(v.h, Dv, w.a2v.q_w, w.a2v.q_b, v_q, Da, v.N, Da, Dv), EPI_BF16, st));
    {
        const float* wts[1] = {w.a2v.qn};
        TRY(qknorm_rope_launch(v_q, Da, v.N, Da, hd, 1, offs, wts, eps, v.ccos, v.csin, st));
    }
    // ---- audio side, side stream: both modulations of ax, a2v K / V, v2a Q ----
    {
        const float* sct[2] = {ta, ta + 2 * Da};
        const float* sht[2] = {ta + Da, ta + 3 * Da};
        const float* sce[2] = {comb ? nullptr : a.cross_ss, comb ? nullptr : a.cross_ss + 2 * Da};
        const float* she[2] = {comb ? nullptr : a.cross_ss + Da, comb ? nullptr : a.cross_ss + 3 * Da};
        TRY(norm_mod2_launch(a.x, Da, a.h, a.h2, Da, a.N, Da, eps, sct, sht, sce, she, sa));       // a2v context side | v2a query side
    }
    TRY(project_kv(c, gemm_dense_params(a.h, Da, w.a2v.kv_w, w.a2v.kv_b, a_kv, 2 * Da, a.N, 2 * Da, Da), a.vt, a.Npad, hd, w.a2v.kn, a.ccos, a.csin, sa));
    hipEvent_t audio_kv = event_record(c, sa);
    if (!audio_kv) return LTX2_E_HIP;
    TRY(gate_logits(c, a, w.v2a, a.h2, Da, a.N, H, sa));
    TRY(dense(c, gemm_dense_params(a.h2, Da, w.v2a.q_w, w.v2a.q_b, a_q, Da, a.N, Da, Da), EPI_BF16, sa));
    {
        const float* wts[1] = {w.v2a.qn};
        TRY(qknorm_rope_launch(a_q, Da, a.N, Da, hd, 1, offs, wts, eps, a.ccos, a.csin, sa));
    }
    // ---- audio -> video attention (main): Q from video, K / V from audio ----
    TRY(event_wait(audio_kv, st));
    TRY(attend(attn_params(v_q, Da, a_kv, 2 * Da, a.vt, a.Npad, v.att, Da, v.N, a.N, H, hd, scale_log2e(hd)), glog(c, v), st));
    {
        GemmParams p = gemm_dense_params(v.att, Da, w.a2v.o_w, w.a2v.o_b, v.x, Dv, v.N, Dv, Da);
        gemm_set_gate(p, comb ? nullptr : v.cross_gate, 0, tv + 4 * Dv);
        TRY(dense(c, p, EPI_RESID_GATE_F32, st));
    }
    // ---- video -> audio attention (side): Q from audio, K / V from video ----
    TRY(event_wait(video_norm, sa));
    {
        GemmParams p = gemm_dense_params(v.h2, Dv, w.v2a.kv_w, w.v2a.kv_b, v_kv, 2 * Da, v.N, 2 * Da, Dv);
        gemm_set_vt(p, v.vt, Da, v.Npad, hd);
        TRY(dense(c, p, EPI_BF16, sa, /*preq=*/false, &vt_done));
    }
    {
        const float* wts[1] = {w.v2a.kn};
        TRY(qknorm_rope_launch(v_kv, 2 * Da, v.N, Da, hd, 1, offs, wts, eps, v.ccos, v.csin, sa));
    }
    if (!vt_done) TRY(vt_transpose_launch(v_kv + Da, 2 * Da, v.vt, v.N, v.Npad, H, sa, hd));
    TRY(attend(attn_params(a_q, Da, v_kv, 2 * Da, v.vt, v.Npad, a.att, Da, a.N, v.N, H, hd, scale_log2e(hd)), glog(c, a), sa));     // few queries, long KV (side stream)
    GemmParams po = gemm_dense_params(a.att, Da, w.v2a.o_w, w.v2a.o_b, a.x, Da, a.N, Da, Da);
    gemm_set_gate(po, comb ? nullptr : a.cross_gate, 0, ta + 4 * Da);
    return dense(c, po, EPI_RESID_GATE_F32, sa);
}

struct ModIn {
    const float* latent;
    const float* ts;       // n_ts timesteps (device)
    int n_ts;
    const float* sigma;    // 1 float (device): this modality's scalar sigma (prompt / cross AdaLN)
    float* velocity;
};

// perturbed: the layers of c->stg[k] run without their self-attention (block_attention()); everything else, the schedule included, is the same program
// isolated (AudioVideo; the reference's SKIP_A2V_CROSS_ATTN + SKIP_V2A_CROSS_ATTN over every block): no layer runs block_cross_modal().  That call
// records and waits all four of its events itself, so leaving the WHOLE call out leaves no wait on an unrecorded event; both joins per layer, the
// early text K / V, the cross-modal AdaLN chains at the top (without a consumer in this pass) and the output heads are the same program
int forward(ltx2_dit* c, const ModIn* in, hipStream_t st, bool rewind_events = true, bool perturbed = false, bool isolated = false) {
    const int nm = c->av ? 2 : 1;
    const auto skip = [&](int k, int l) { return perturbed && !c->stg[k].empty() && c->stg[k][l] != 0; };
    if (rewind_events) c->sync_next = 0;
    long es[2] = {0, 0}, ee[2] = {0, 0};
    for (int k = 0; k < nm; ++k) {
        Mod& m = c->m[k];
        const ModW& w = c->mw[k];
        LTX2_CHECK_ARG(in[k].n_ts == 1 || in[k].n_ts == m.N, "dit_forward: n_timesteps=%d must be 1 or N=%d", in[k].n_ts, m.N);
        LTX2_CHECK_ARG(in[k].n_ts == 1 || c->per_token, "dit_forward: workspace was not sized for per-token timesteps");
        // patchify_proj (model.py:242) -> fp32 residual stream
        TRY(cast_f32_bf16_launch(in[k].latent, m.lat, (long)m.N * m.Cin, st));
        TRY(dense(c, gemm_dense_params(m.lat, m.Cin, w.patch_w, w.patch_b, m.x, m.D, m.N, m.D, m.Cin), EPI_F32, st));
        // AdaLN-single (model.py:113-140)
        TRY(adaln_chain(c, m, w.ada, in[k].ts, 1, in[k].n_ts, c->cfg.timestep_scale, m.emb, m.e_f, st));
        if (in[k].n_ts > 1) {
            es[k] = (long)w.ada.rows * m.D;
            ee[k] = m.D;
        } else if (c->adaln_combine) {
            // one timestep for the whole modality (every loop but the conditioned ones): table + embedding of all layers in one launch; the
            // blocks then pass the sums as tables (rows_of()), the norm kernels read half the vectors and the gated-residual GEMMs no per-row gate
            TRY(adaln_combine_launch(m.sst_all, m.emb, m.comb, c->cfg.num_layers, (long)w.ada.rows * m.D, st));
        }
        m.use_comb = in[k].n_ts == 1 && c->adaln_combine;
        if (c->v2)           // prompt AdaLN from this modality's sigma (model.py:151-161)
            TRY(adaln_chain(c, m, w.prompt, in[k].sigma, 0, 1, c->cfg.timestep_scale, m.prompt_emb, nullptr, st));
        if (c->av) {         // cross-modal AdaLN from the OTHER modality's sigma (model.py:346-364,392-404)
            const float* cs = in[1 - k].sigma;
            TRY(adaln_chain(c, m, w.cross_ss, cs, 0, 1, c->cfg.timestep_scale, m.cross_ss, nullptr, st));
            TRY(adaln_chain(c, m, w.cross_gate, cs, 0, 1, c->cfg.av_ca_timestep_scale, m.cross_gate, nullptr, st));
            if (c->adaln_combine) {      // the five cross-modal rows (scale / shift x 2, gate) of every layer + their embeddings (cross_ss | cross_gate are adjacent)
                LTX2_CHECK_ARG(m.cross_gate == m.cross_ss + 4L * m.D, "dit_forward: cross-modal embedding rows are not contiguous");
                TRY(adaln_combine_launch(m.ca_all, m.cross_ss, m.ca_comb, c->cfg.num_layers, 5L * m.D, st));
            }
        }
    }
    // round 6: the text cross-attention's pre-norm folded around its GEMMs (block_attention()): row-invariant gates only
    const int fold = (!c->av && c->m[0].use_comb && c->fold_norms >= 1 && c->m[0].fold_max >= 1) ? 1 : 0;
    // the audio modality's block program runs on the side stream, joined around the cross-modal attention
    hipStream_t sa = (c->av && c->side) ? c->side : st;
    c->text_kv_ev = nullptr;
    for (int l = 0; l < c->cfg.num_layers; ++l) {
        if (c->av) {
            TRY(stream_after(c, st, sa));
            // the side stream has just waited for everything of layer l - 1 (its text cross-attention read kv2 / vt2: free now); the video stream's
            // text K / V of THIS layer go first on it, beside the main stream's norm / gate / QKV projection
            // (not with fp8 compute: that projection quantises its input into the video modality's ONE activation scratch, which the main stream is using)
            if (c->v2 && c->text_kv_ahead && sa != st && !c->fp8_compute) {
                TRY(text_kv(c, 0, l, sa));
                c->text_kv_ev = event_record(c, sa);
                if (!c->text_kv_ev) return LTX2_E_HIP;
            }
            TRY(block_attention(c, 1, l, es[1], sa, 0, skip(1, l)));
        }
        TRY(block_attention(c, 0, l, es[0], st, fold, skip(0, l)));
        if (c->av) {
            if (!isolated) TRY(block_cross_modal(c, l, st, sa));      // main: the video side; side: the audio side (events inside)
            TRY(block_ffn(c, 1, l, es[1], sa));
        }
        TRY(block_ffn(c, 0, l, es[0], st));
        if (c->av) TRY(stream_after(c, sa, st));
    }
    // output heads (model.py:744-774): LayerNorm(no affine) * (1 + scale) + shift, rows (shift, scale)
    for (int k = 0; k < nm; ++k) {
        Mod& m = c->m[k];
        const ModW& w = c->mw[k];
        TRY(norm_mod_launch(m.x, m.D, m.h, m.D, m.N, m.D, c->cfg.norm_eps, 1, w.sst_out + m.D, w.sst_out, m.e_f, m.e_f, ee[k], st));
        TRY(dense(c, gemm_dense_params(m.h, m.D, w.proj_w, w.proj_b, in[k].velocity, m.Cout, m.N, m.Cout, m.D), EPI_F32, st));
    }
    return LTX2_OK;
}

struct StepIo {
    float* latent;
    const float* mask;
    const float* clean;
    float* x0_out;
};

int denoise_step(ltx2_dit* c, ModIn* in, const StepIo* io, float sigma, float sigma_next, hipStream_t st,
                 bool rewind_events = true) {
    const int nm = c->av ? 2 : 1;
    for (int k = 0; k < nm; ++k) {
        in[k].latent = io[k].latent;
        in[k].velocity = c->m[k].vel;
    }
    TRY(forward(c, in, st, rewind_events));
    for (int k = 0; k < nm; ++k) {
        Mod& m = c->m[k];
        float* x0 = io[k].x0_out ? io[k].x0_out : m.x0;
        TRY(x0_from_velocity_launch(io[k].latent, m.vel, in[k].ts, in[k].n_ts == 1 ? 0 : 1, 0.f, x0, m.N, m.Cout, st));
        TRY(euler_step_launch(io[k].latent, x0, io[k].mask, io[k].clean, sigma, sigma_next, io[k].latent, m.N, m.Cout, st));
    }
    return LTX2_OK;
}

int prepare_modality(ltx2_dit* c, int k, const float* context, int S, const float* cosb, const float* sinb,
                     const float* ccos, const float* csin, hipStream_t st) {
    Mod& m = c->m[k];
    const ModW& w = c->mw[k];
    LTX2_CHECK_ARG(context && cosb && sinb, "dit_prepare: null argument");
    LTX2_CHECK_ARG(S == m.S, "dit_prepare: S=%d differs from the bound workspace S=%d", S, m.S);
    const int D = m.D;
    const int Cctx = c->cfg.caption_channels > 0 ? c->cfg.caption_channels : D;
    bool ok = hipMemcpyAsync(m.cosb, cosb, 4L * m.N * (D / 2), hipMemcpyDeviceToDevice, st) == hipSuccess &&
              hipMemcpyAsync(m.sinb, sinb, 4L * m.N * (D / 2), hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (c->av) {
        LTX2_CHECK_ARG(ccos && csin, "dit_prepare: cross-modal RoPE tables are required for AudioVideo models");
        const long Dc = c->m[1].D;
        ok = ok && hipMemcpyAsync(m.ccos, ccos, 4L * m.N * (Dc / 2), hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(m.csin, csin, 4L * m.N * (Dc / 2), hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
    if (!ok) {
        ltx2_set_error("dit_prepare: RoPE table copy failed");
        return LTX2_E_HIP;
    }
    TRY(cast_f32_bf16_launch(context, m.ctx_in, (long)S * Cctx, st));
    m.ctx = m.ctx_in;
    if (c->cfg.caption_channels > 0) {   // PixArtAlphaTextProjection (model.py:52-56)
        TRY(dense(c, gemm_dense_params(m.ctx_in, Cctx, w.cap1_w, w.cap1_b, m.c1, D, S, D, Cctx), EPI_GELU_BF16, st));
        TRY(dense(c, gemm_dense_params(m.c1, D, w.cap2_w, w.cap2_b, m.ctxp, D, S, D, D), EPI_BF16, st));
        m.ctx = m.ctxp;
    }
    {   // every layer's scale_shift_table side by side: forward() adds the step's timestep embedding to all of them in one launch
        const long n = (long)(c->v2 ? 9 : 6) * D;
        for (int l = 0; l < c->cfg.num_layers; ++l)
            if (hipMemcpyAsync(m.sst_all + l * n, c->layers[l].m[k].sst, 4L * n, hipMemcpyDeviceToDevice, st) != hipSuccess) {
                ltx2_set_error("dit_prepare: scale_shift_table copy failed");
                return LTX2_E_HIP;
            }
    }
    if (c->av)
        for (int l = 0; l < c->cfg.num_layers; ++l)
            if (hipMemcpyAsync(m.ca_all + (long)l * 5 * D, c->layers[l].ca[k], 4L * 5 * D, hipMemcpyDeviceToDevice, st) != hipSuccess) {
                ltx2_set_error("dit_prepare: cross-modal scale_shift_table copy failed");
                return LTX2_E_HIP;
            }
    m.fold_max = fold_supported(c, k);
    m.qfold = text_qfold_ok(c, k);
    if (m.qfold)
        for (int l = 0; l < c->cfg.num_layers; ++l) {
            const AttnW& tw = c->layers[l].m[k].text;
            hipLaunchKernelGGL(vec_mul_kernel, dim3((D + 255) / 256), dim3(256), 0, st, tw.kn, tw.qn, m.knq + (long)l * D, D);
        }
    if (!c->v2)
        for (int l = 0; l < c->cfg.num_layers; ++l) {
            const AttnW& tw = c->layers[l].m[k].text;
            TRY(project_kv(c, gemm_dense_params(m.ctx, D, tw.kv_w, tw.kv_b, m.kv2 + (long)l * S * 2 * D, 2 * D, S, 2 * D, D), m.vt2 + (long)l * D * m.Spad,
                           m.Spad, m.hd, m.qfold ? m.knq + (long)l * D : tw.kn, nullptr, nullptr, st));
        }
    return LTX2_OK;
}

// host_sub: n_steps sub-sigmas uploaded behind the 64 sigma slots (the res_2s loop), or nullptr
int begin_capture(ltx2_dit* c, const float* host_sigmas, int n_steps, hipStream_t st, const float* host_sub = nullptr) {
    LTX2_CHECK_ARG(st != nullptr, "dit_graph_capture: needs a non-default stream");
    for (int i = 0; i < n_steps; ++i) LTX2_CHECK_ARG(host_sigmas[i] != 0.f, "Sigma can't be 0.0");
    if (hipMemcpyAsync(c->sigmas_dev, host_sigmas, 4L * (n_steps + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        (host_sub && hipMemcpyAsync(c->sigmas_dev + 64, host_sub, 4L * n_steps, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess) {
        ltx2_set_error("dit_graph_capture: sigma upload failed");
        return LTX2_E_HIP;
    }
    if (c->exec) {
        (void)hipGraphExecDestroy(c->exec);
        c->exec = nullptr;
    }
    if (c->graph) {
        (void)hipGraphDestroy(c->graph);
        c->graph = nullptr;
    }
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        ltx2_set_error("dit_graph_capture: hipStreamBeginCapture failed");
        return LTX2_E_HIP;
    }
    return LTX2_OK;
}

int end_capture(ltx2_dit* c, int rc, hipStream_t st) {
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != LTX2_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) {
        ltx2_set_error("dit_graph_capture: hipStreamEndCapture failed: %s", hipGetErrorString(e));
        return LTX2_E_HIP;
    }
    c->graph = g;
    if (hipGraphInstantiate(&c->exec, g, nullptr, nullptr, 0) != hipSuccess) {
        ltx2_set_error("dit_graph_capture: hipGraphInstantiate failed");
        return LTX2_E_HIP;
    }
    return LTX2_OK;
}

int check_ready(ltx2_dit* c, const char* who, bool want_av) {
    LTX2_CHECK_ARG(c, "%s: null context", who);
    LTX2_CHECK_ARG(c->av == want_av, "%s: model is %s", who, c->av ? "AudioVideo (use the *_av entry points)" : "VideoOnly");
    if (!c->prepared) {
        ltx2_set_error("%s: ltx2_dit_prepare has not been called", who);
        return LTX2_E_STATE;
    }
    return LTX2_OK;
}

int bind(ltx2_dit* c, void* ptr, int64_t bytes, int N, int S, int Na, int Sa, int per_token) {
    LTX2_CHECK_ARG(((uintptr_t)ptr & 255) == 0, "dit_bind_workspace: pointer must be 256-byte aligned");
    const long need = carve(c, (char*)ptr, N, S, Na, Sa, per_token);
    if (bytes < need) {
        ltx2_set_error("dit_bind_workspace: %ld bytes given, %ld needed", (long)bytes, need);
        return LTX2_E_STATE;
    }
    c->ws = (char*)ptr;
    c->ws_bytes = bytes;
    const int n[2] = {N, Na}, s[2] = {S, Sa};
    for (int k = 0; k < 2; ++k) {
        c->m[k].N = n[k];
        c->m[k].S = s[k];
        c->m[k].Npad = (int)align_up(n[k], 64);
        c->m[k].Spad = (int)align_up(s[k], 64);
    }
    c->per_token = per_token;
    c->prepared = false;
    c->m[0].has_kmask = c->m[1].has_kmask = false;
    return LTX2_OK;
}

}  // namespace

extern "C" {

int ltx2_dit_create(const ltx2_dit_config* cfg, ltx2_dit** out) {
    LTX2_CHECK_ARG(cfg && out, "dit_create: null argument");
    LTX2_CHECK_ARG(cfg->head_dim == 128 || cfg->head_dim == 64, "dit_create: head_dim=%d, only 128 and 64 are implemented", cfg->head_dim);
    LTX2_CHECK_ARG(cfg->num_layers > 0 && cfg->num_heads > 0, "dit_create: bad layer/head count");
    LTX2_CHECK_ARG(cfg->in_channels % 64 == 0, "dit_create: in_channels must be a multiple of 64");
    LTX2_CHECK_ARG(cfg->caption_channels % 64 == 0, "dit_create: caption_channels must be a multiple of 64");
    LTX2_CHECK_ARG(cfg->model_type == LTX2_MODEL_VIDEO_ONLY || cfg->model_type == LTX2_MODEL_AUDIO_VIDEO, "dit_create: bad model_type %d", cfg->model_type);
    ltx2_dit* c = new ltx2_dit();
    c->cfg = *cfg;
    c->av = cfg->model_type == LTX2_MODEL_AUDIO_VIDEO;
    c->v2 = cfg->cross_attention_adaln != 0;
    c->gated = cfg->apply_gated_attention != 0;
    Mod& v = c->m[0];
    v.H = cfg->num_heads;
    v.hd = cfg->head_dim;
    v.D = v.H * v.hd;
    v.Cin = cfg->in_channels;
    v.Cout = cfg->out_channels;
    if (c->av) {
        if (!(cfg->audio_head_dim == 64 && cfg->audio_heads == cfg->num_heads && cfg->audio_in_channels % 64 == 0)) {
            delete c;
            ltx2_set_error("dit_create: AudioVideo needs audio_head_dim = 64, audio_heads = num_heads (shared cross-modal RoPE heads) and audio_in_channels %% 64 == 0");
            return LTX2_E_INVALID;
        }
        Mod& a = c->m[1];
        a.H = cfg->audio_heads;
        a.hd = cfg->audio_head_dim;
        a.D = a.H * a.hd;
        a.Cin = cfg->audio_in_channels;
        a.Cout = cfg->audio_out_channels;
    }
    if (c->av) {
        // (round 4: a high-priority side stream measured the same as the default priority, eager and under hipGraph; a LOW priority one 144 vs 105 ms
        // eager -- the audio chain then starves behind the video GEMMs' queued tiles)
        const bool ok = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) == hipSuccess;
        if (!ok) {
            ltx2_set_error("dit_create: side stream / event creation failed");
            return LTX2_E_HIP;
        }
    }
    *out = c;
    return LTX2_OK;
}

void ltx2_dit_destroy(ltx2_dit* c) {
    if (!c) return;
    for (hipEvent_t e : c->sync_ev) (void)hipEventDestroy(e);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->r2s) (void)hipFree(c->r2s);
    if (c->heun) (void)hipFree(c->heun);
    if (c->pg_part) (void)hipFree(c->pg_part);
    if (c->pg_run) (void)hipFree(c->pg_run);
    for (double* p : c->mm_part)
        if (p) (void)hipFree(p);
    for (double* p : c->pgj_part)
        if (p) (void)hipFree(p);
    if (c->cs_part) (void)hipFree(c->cs_part);
    if (c->xattn_gate) (void)hipFree(c->xattn_gate);
    if (c->exec) (void)hipGraphExecDestroy(c->exec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    delete c;
}

int ltx2_dit_set_weight(ltx2_dit* c, const char* name, const void* ptr, int dtype, int64_t numel) {
    LTX2_CHECK_ARG(c && name && ptr, "dit_set_weight: null argument");
    LTX2_CHECK_ARG(dtype == LTX2_DTYPE_BF16 || dtype == LTX2_DTYPE_F32 || dtype == LTX2_DTYPE_FP8_E4M3FN, "dit_set_weight: bad dtype %d", dtype);
    c->weights[name] = Wt{ptr, dtype, (long)numel};
    c->resolved = false;
    c->prepared = false;        // the per-prompt caches (text K/V, the gathered AdaLN tables) were built from the weights registered before
    return LTX2_OK;
}

int64_t ltx2_dit_workspace_bytes_av(const ltx2_dit* c, int N, int S, int Na, int Sa, int per_token) {
    if (!c || N <= 0 || S <= 0 || (c->av && (Na <= 0 || Sa <= 0))) return -1;
    ltx2_dit tmp;            // carve() writes pointers; use a scratch context
    tmp.cfg = c->cfg;
    tmp.av = c->av;
    tmp.v2 = c->v2;
    tmp.gated = c->gated;
    tmp.fp8_compute = c->fp8_compute;
    tmp.m[0] = c->m[0];
    tmp.m[1] = c->m[1];
    return carve(&tmp, nullptr, N, S, Na, Sa, per_token);
}

int64_t ltx2_dit_workspace_bytes(const ltx2_dit* c, int N, int S, int per_token) {
    if (!c || c->av) return -1;
    return ltx2_dit_workspace_bytes_av(c, N, S, 0, 0, per_token);
}

int ltx2_dit_bind_workspace(ltx2_dit* c, void* ptr, int64_t bytes, int N, int S, int per_token) {
    LTX2_CHECK_ARG(c && ptr && N > 0 && S > 0, "dit_bind_workspace: bad argument");
    LTX2_CHECK_ARG(!c->av, "dit_bind_workspace: AudioVideo model, use ltx2_dit_bind_workspace_av");
    return bind(c, ptr, bytes, N, S, 0, 0, per_token);
}

int ltx2_dit_bind_workspace_av(ltx2_dit* c, void* ptr, int64_t bytes, int N, int S, int Na, int Sa, int per_token) {
    LTX2_CHECK_ARG(c && ptr && N > 0 && S > 0 && Na > 0 && Sa > 0, "dit_bind_workspace_av: bad argument");
    LTX2_CHECK_ARG(c->av, "dit_bind_workspace_av: VideoOnly model, use ltx2_dit_bind_workspace");
    return bind(c, ptr, bytes, N, S, Na, Sa, per_token);
}

int ltx2_dit_prepare(ltx2_dit* c, const float* context, int S, const float* rope_cos, const float* rope_sin,
                     void* stream) {
    LTX2_CHECK_ARG(c, "dit_prepare: null context");
    LTX2_CHECK_ARG(!c->av, "dit_prepare: AudioVideo model, use ltx2_dit_prepare_av");
    if (!c->ws) {
        ltx2_set_error("dit_prepare: no workspace bound");
        return LTX2_E_STATE;
    }
    TRY(resolve(c));
    TRY(prepare_modality(c, 0, context, S, rope_cos, rope_sin, nullptr, nullptr, (hipStream_t)stream));
    c->prepared = true;
    return LTX2_OK;
}

int ltx2_dit_prepare_av(ltx2_dit* c, const float* v_context, int S, const float* v_cos, const float* v_sin,
                        const float* v_cross_cos, const float* v_cross_sin, const float* a_context, int Sa,
                        const float* a_cos, const float* a_sin, const float* a_cross_cos, const float* a_cross_sin,
                        void* stream) {
    LTX2_CHECK_ARG(c, "dit_prepare_av: null context");
    LTX2_CHECK_ARG(c->av, "dit_prepare_av: VideoOnly model, use ltx2_dit_prepare");
    if (!c->ws) {
        ltx2_set_error("dit_prepare_av: no workspace bound");
        return LTX2_E_STATE;
    }
    TRY(resolve(c));
    TRY(prepare_modality(c, 0, v_context, S, v_cos, v_sin, v_cross_cos, v_cross_sin, (hipStream_t)stream));
    TRY(prepare_modality(c, 1, a_context, Sa, a_cos, a_sin, a_cross_cos, a_cross_sin, (hipStream_t)stream));
    c->prepared = true;
    return LTX2_OK;
}

int ltx2_dit_forward(ltx2_dit* c, const float* latent, const float* timesteps, int n_timesteps, const float* sigma,
                     float* velocity, void* stream) {
    LTX2_CHECK_ARG(latent && timesteps && velocity, "dit_forward: null argument");
    TRY(check_ready(c, "dit_forward", false));
    ModIn in[1] = {{latent, timesteps, n_timesteps, sigma ? sigma : timesteps, velocity}};
    return forward(c, in, (hipStream_t)stream);
}

int ltx2_dit_forward_av(ltx2_dit* c, const float* v_latent, const float* v_timesteps, int n_v_timesteps,
                        const float* v_sigma, const float* a_latent, const float* a_timesteps, int n_a_timesteps,
                        const float* a_sigma, float* v_velocity, float* a_velocity, void* stream) {
    LTX2_CHECK_ARG(v_latent && v_timesteps && v_sigma && a_latent && a_timesteps && a_sigma && v_velocity && a_velocity,
                   "dit_forward_av: null argument");
    TRY(check_ready(c, "dit_forward_av", true));
    ModIn in[2] = {{v_latent, v_timesteps, n_v_timesteps, v_sigma, v_velocity},
                   {a_latent, a_timesteps, n_a_timesteps, a_sigma, a_velocity}};
    return forward(c, in, (hipStream_t)stream);
}

int ltx2_dit_set_stg_blocks(ltx2_dit* c, int modality, const unsigned char* flags, int n_layers) {
    LTX2_CHECK_ARG(c && (modality == 0 || (modality == 1 && c->av)), "dit_set_stg_blocks: bad context / modality");
    if (!flags) {
        c->stg[modality].clear();
        return LTX2_OK;
    }
    LTX2_CHECK_ARG(n_layers == c->cfg.num_layers, "dit_set_stg_blocks: n_layers=%d, the model has %d", n_layers, c->cfg.num_layers);
    c->stg[modality].assign(flags, flags + n_layers);
    return LTX2_OK;
}

int ltx2_dit_set_cross_attn_scale(ltx2_dit* c, float scale, int start_layer) {
    LTX2_CHECK_ARG(c && start_layer >= 0, "dit_set_cross_attn_scale: bad argument");
    if (c->av || c->v2) {       // there the text cross-attention's gate is per row (AdaLN row 8), not a table; scaling it is not built
        ltx2_set_error("dit_set_cross_attn_scale: built for the VideoOnly LTX-2.0 model alone (a gated text cross-attention and AudioVideo models are not)");
        return LTX2_E_UNSUPPORTED;
    }
    c->xattn_on = false;
    if (scale == 1.0f) return LTX2_OK;          // the launch goes without a table again; the buffer stays until the context goes (a captured graph may name it)
    const int D = c->m[0].D;
    if (!c->xattn_gate && hipMalloc((void**)&c->xattn_gate, 4L * D) != hipSuccess) {
        c->xattn_gate = nullptr;
        ltx2_set_error("dit_set_cross_attn_scale: allocating %ld bytes failed", 4L * D);
        return LTX2_E_HIP;
    }
    const std::vector<float> table(D, scale);
    if (hipMemcpy(c->xattn_gate, table.data(), 4L * D, hipMemcpyHostToDevice) != hipSuccess) {
        ltx2_set_error("dit_set_cross_attn_scale: hipMemcpy failed");
        return LTX2_E_HIP;
    }
    c->xattn_start = start_layer;
    c->xattn_on = true;
    return LTX2_OK;
}

int ltx2_dit_forward_perturbed(ltx2_dit* c, const float* latent, const float* timesteps, int n_timesteps, const float* sigma,
                               float* velocity, void* stream) {
    LTX2_CHECK_ARG(latent && timesteps && velocity, "dit_forward_perturbed: null argument");
    TRY(check_ready(c, "dit_forward_perturbed", false));
    ModIn in[1] = {{latent, timesteps, n_timesteps, sigma ? sigma : timesteps, velocity}};
    return forward(c, in, (hipStream_t)stream, true, true);
}

int ltx2_dit_forward_perturbed_av(ltx2_dit* c, const float* v_latent, const float* v_timesteps, int n_v_timesteps,
                                  const float* v_sigma, const float* a_latent, const float* a_timesteps, int n_a_timesteps,
                                  const float* a_sigma, float* v_velocity, float* a_velocity, void* stream) {
    LTX2_CHECK_ARG(v_latent && v_timesteps && v_sigma && a_latent && a_timesteps && a_sigma && v_velocity && a_velocity,
                   "dit_forward_perturbed_av: null argument");
    TRY(check_ready(c, "dit_forward_perturbed_av", true));
    ModIn in[2] = {{v_latent, v_timesteps, n_v_timesteps, v_sigma, v_velocity},
                   {a_latent, a_timesteps, n_a_timesteps, a_sigma, a_velocity}};
    return forward(c, in, (hipStream_t)stream, true, true);
}

int ltx2_dit_forward_isolated_av(ltx2_dit* c, const float* v_latent, const float* v_timesteps, int n_v_timesteps,
                                 const float* v_sigma, const float* a_latent, const float* a_timesteps, int n_a_timesteps,
                                 const float* a_sigma, float* v_velocity, float* a_velocity, void* stream) {
    LTX2_CHECK_ARG(v_latent && v_timesteps && v_sigma && a_latent && a_timesteps && a_sigma && v_velocity && a_velocity,
                   "dit_forward_isolated_av: null argument");
    TRY(check_ready(c, "dit_forward_isolated_av", true));
    ModIn in[2] = {{v_latent, v_timesteps, n_v_timesteps, v_sigma, v_velocity},
                   {a_latent, a_timesteps, n_a_timesteps, a_sigma, a_velocity}};
    return forward(c, in, (hipStream_t)stream, true, false, true);
}

int ltx2_dit_denoise_step(ltx2_dit* c, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                          const float* mask, const float* clean, float sigma, float sigma_next, float* x0_out, void* stream) {
    LTX2_CHECK_ARG(latent && timesteps, "dit_denoise_step: null argument");
    TRY(check_ready(c, "dit_denoise_step", false));
    ModIn in[1] = {{latent, timesteps, n_timesteps, sigma_dev ? sigma_dev : timesteps, nullptr}};
    const StepIo io[1] = {{latent, mask, clean, x0_out}};
    return denoise_step(c, in, io, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_denoise_step_av(ltx2_dit* c, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                             const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask,
                             const float* v_clean, const float* a_mask, const float* a_clean, float sigma,
                             float sigma_next, float* v_x0_out, float* a_x0_out, void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_denoise_step_av: null argument");
    TRY(check_ready(c, "dit_denoise_step_av", true));
    ModIn in[2] = {{v_latent, v_timesteps, n_v_timesteps, sigma_dev, nullptr},
                   {a_latent, a_timesteps, n_a_timesteps, sigma_dev, nullptr}};
    const StepIo io[2] = {{v_latent, v_mask, v_clean, v_x0_out}, {a_latent, a_mask, a_clean, a_x0_out}};
    return denoise_step(c, in, io, sigma, sigma_next, (hipStream_t)stream);
}

// Conditioned loops (image-to-video: some tokens carry a denoise mask < 1): per step the timesteps are mask * sigma_i, formed on the device
// inside the captured step, and the Euler update blends x0 with the clean latent as ltx2_dit_denoise_step does.
namespace {
struct Cond {       // one modality's conditioning of a captured loop; mask == nullptr: none (the uniform form)
    const float* mask;
    long n_mask;
    const float* clean;
    long n_clean;
};

// blend = false: a modality that is evaluated but never stepped (the frozen audio of the AudioVideo guided loop): the timesteps alone, no clean latent
int cond_modality(ltx2_dit* c, int k, const Cond& cd, const float* sigma_i, ModIn& in, StepIo& io, hipStream_t st, bool blend = true) {
    Mod& m = c->m[k];
    if (!cd.mask) return LTX2_OK;
    LTX2_CHECK_ARG(cd.clean || !blend, "dit_graph_capture_cond: a denoise mask needs the clean latent");
    // the replayed kernels read N mask elements and N * C clean-latent elements on every step: a buffer of another modality's length would be an
    // out-of-bounds device read, not an error
    LTX2_CHECK_ARG(cd.n_mask == m.N && (!blend || cd.n_clean == (long)m.N * m.Cout), "dit_graph_capture_cond: modality %d has %d tokens x %d channels, got a mask of %ld and a clean latent of %ld elements", k, m.N, m.Cout, cd.n_mask, cd.n_clean);
    if (!c->per_token || !m.ts_tok) {
        ltx2_set_error("dit_graph_capture_cond: the workspace was not bound for per-token timesteps");
        return LTX2_E_STATE;
    }
    hipLaunchKernelGGL(mask_sigma_kernel, dim3((m.N + 255) / 256), dim3(256), 0, st, cd.mask, sigma_i, m.ts_tok, m.N);
    LTX2_CHECK_LAUNCH("mask_sigma_kernel");
    in.ts = m.ts_tok;
    in.n_ts = m.N;
    if (!blend) return LTX2_OK;
    io.mask = cd.mask;
    io.clean = cd.clean;
    return LTX2_OK;
}

// ---- The shared path of every guided and every second-order step -------------------------------------------------------------------------------------
// A step entry, or the capture entry of a loop of such steps, asks step_ready() once, before anything is enqueued.  The step then evaluates its inputs
// through the positive prompt's context `c` and, where there is one, through `neg` (the negative prompt: a second context over the same weights, with its
// own text K / V) by evaluate(), and runs its one or two element-wise passes (csrc/sampler.hip).  Everything goes onto the caller's stream in order: each
// evaluation already fills the device, so a captured loop is a linear chain.  VideoOnly contexts (an AudioVideo model's video twin) have one modality,
// in[0] / io[0]; AudioVideo contexts two.

// n_ts[k]: the timesteps the step passes for modality k.  neg may be NULL: no guidance (the entries that need one check that themselves).
int step_ready(ltx2_dit* c, ltx2_dit* neg, bool want_av, const int n_ts[2], const char* who) {
    LTX2_CHECK_ARG(c, "%s: null context", who);
    LTX2_CHECK_ARG(c != neg, "%s: the negative prompt needs a context of its own (ctx == neg)", who);
    LTX2_CHECK_ARG(c->av == want_av && (!neg || neg->av == want_av), "%s: %s", who,
                   want_av ? "every context must be AudioVideo (the VideoOnly engine has the entry without _av)"
                           : "the step runs on VideoOnly contexts (the video twin of an AudioVideo model)");
    LTX2_CHECK_ARG(c->prepared && (!neg || neg->prepared), "%s: ltx2_dit_prepare%s has not been called on every context", who, want_av ? "_av" : "");
    const int nm = want_av ? 2 : 1;
    for (int k = 0; neg && k < nm; ++k)
        LTX2_CHECK_ARG(c->m[k].N == neg->m[k].N && c->m[k].Cout == neg->m[k].Cout, "%s: the contexts differ in modality %d: %d tokens x %d channels against %d x %d",
                       who, k, c->m[k].N, c->m[k].Cout, neg->m[k].N, neg->m[k].Cout);
    bool per_token = false;
    for (int k = 0; k < nm; ++k) {
        LTX2_CHECK_ARG(n_ts[k] == 1 || n_ts[k] == c->m[k].N, "%s: n_timesteps=%d of modality %d must be 1 or %s=%d", who, n_ts[k], k, k ? "Na" : "N", c->m[k].N);
        per_token = per_token || n_ts[k] != 1;
    }
    LTX2_CHECK_ARG(!per_token || (c->per_token && (!neg || neg->per_token)), "%s: a workspace was not bound for per-token timesteps", who);
    return LTX2_OK;
}

// One evaluation of in[k] = (latent, timesteps, sigma) of every modality through c into c's velocity buffers and, with a negative context, a second
// through neg into neg's.  rewind_events: forward()'s; only an AudioVideo forward takes events, so inside a capture those loops pass i == 0.
int evaluate(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, hipStream_t st, bool rewind_events = true) {
    ltx2_dit* const both[2] = {c, neg};
    for (ltx2_dit* e : both) {
        if (!e) continue;
        ModIn ev[2] = {};
        for (int k = 0; k < (c->av ? 2 : 1); ++k) {
            ev[k] = in[k];
            ev[k].velocity = e->m[k].vel;
        }
        TRY(forward(e, ev, st, rewind_events));
    }
    return LTX2_OK;
}

// What the step entries build from their arguments: (latent, timesteps, sigma) of one modality and the latent the step updates with its conditioning
struct StepArgs {
    ModIn in;
    StepIo io;
};

StepArgs step_args(float* latent, const float* ts, int n_ts, const float* sigma_dev, const float* mask, const float* clean) {
    return {{latent, ts, n_ts, sigma_dev ? sigma_dev : ts, nullptr}, {latent, mask, clean, nullptr}};
}

// What every Euler-type step checks of its scalars and its nm conditionings
int step_check(float sigma, const StepIo* io, int nm, const char* who) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");
    for (int k = 0; k < nm; ++k) LTX2_CHECK_ARG((io[k].mask == nullptr) == (io[k].clean == nullptr), "%s: mask and clean go together", who);
    return LTX2_OK;
}

// Classifier-free guidance (keyframe interpolation's stage 1; on AudioVideo contexts audio-to-video, reference pipelines/a2vid_two_stage.py:225-271): two
// evaluations per step, then ONE element-wise pass over modality 0.  An audio latent in[1] is evaluated by both contexts and never stepped.
// io: the video latent the step updates and its conditioning
int guided_step(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const StepIo& io, float cfg_scale, float sigma, float sigma_next, hipStream_t st,
                bool rewind_events = true) {
    TRY(step_check(sigma, &io, 1, "dit_guided_step"));
    const Mod& m = c->m[0];
    TRY(evaluate(c, neg, in, st, rewind_events));
    return guided_euler_step_launch(in[0].latent, m.vel, neg->m[0].vel, in[0].ts, in[0].n_ts == 1 ? 0 : 1, io.mask, io.clean, cfg_scale, sigma, sigma_next,
                                    io.latent, m.N, m.Cout, st);
}

// The same on AudioVideo contexts with BOTH latents stepped (a retake with sound; the reference's pipelines/retake.py:234-291 run with an audio state):
// the two evaluations, then ONE element-wise launch over both latents, the video under cfg[0] and the audio under cfg[1].
int guided_step_joint(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const StepIo* io, const float cfg[2], float sigma, float sigma_next, hipStream_t st,
                      bool rewind_events = true) {
    TRY(step_check(sigma, io, 2, "dit_guided_step_joint_av"));
    const Mod &v = c->m[0], &a = c->m[1];
    TRY(evaluate(c, neg, in, st, rewind_events));
    return guided_euler_step_pair_launch(in[0].latent, v.vel, neg->m[0].vel, in[0].ts, in[0].n_ts == 1 ? 0 : 1, io[0].mask, io[0].clean, cfg[0], io[0].latent,
                                         v.N, v.Cout, in[1].latent, a.vel, neg->m[1].vel, in[1].ts, in[1].n_ts == 1 ? 0 : 1, io[1].mask, io[1].clean, cfg[1],
                                         io[1].latent, a.N, a.Cout, sigma, sigma_next, st);
}

// The Euler-ancestral step (reference components/diffusion_steps.py:70-129) on VideoOnly contexts (in[0] / io[0]) or, on AudioVideo contexts, over BOTH
// latents: the evaluations of guided_step / guided_step_joint (neg NULL: one, no guidance), then ONE element-wise launch that also makes the noise
// (csrc/sampler.hip), the video latent from Philox stream 0 and the audio latent from stream 1.  Every refusal stands before anything is enqueued.
struct Ancestral {
    float up, down;             // _get_ancestral_step(sigma, sigma_next, eta), evaluated by the caller in double
    const uint64_t* seed;       // device, one 64-bit word
    uint32_t step;
};

int ancestral_step(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const StepIo* io, const float cfg[2], float sigma, const Ancestral& an, hipStream_t st,
                   bool rewind_events = true) {
    const char* who = c->av ? "dit_ancestral_step_joint_av" : "dit_ancestral_step";
    TRY(step_check(sigma, io, c->av ? 2 : 1, who));
    LTX2_CHECK_ARG(an.up >= 0.f && an.down >= 0.f, "%s: sigma_up=%g and sigma_down=%g must be >= 0", who, an.up, an.down);
    LTX2_CHECK_ARG(an.seed && ((uintptr_t)an.seed & 7) == 0, "%s: seed_dev is a device pointer to one 8-byte aligned 64-bit word", who);
    const Mod &v = c->m[0], &a = c->m[1];
    TRY(evaluate(c, neg, in, st, rewind_events));
    if (!c->av)
        return ancestral_euler_step_launch(in[0].latent, v.vel, neg ? neg->m[0].vel : nullptr, in[0].ts, in[0].n_ts == 1 ? 0 : 1, io[0].mask, io[0].clean,
                                           cfg[0], sigma, an.up, an.down, an.seed, an.step, io[0].latent, v.N, v.Cout, st);
    return ancestral_euler_step_pair_launch(in[0].latent, v.vel, neg ? neg->m[0].vel : nullptr, in[0].ts, in[0].n_ts == 1 ? 0 : 1, io[0].mask, io[0].clean,
                                            cfg[0], io[0].latent, v.N, v.Cout, in[1].latent, a.vel, neg ? neg->m[1].vel : nullptr, in[1].ts,
                                            in[1].n_ts == 1 ? 0 : 1, io[1].mask, io[1].clean, cfg[1], io[1].latent, a.N, a.Cout, sigma, an.up, an.down,
                                            an.seed, an.step, st);
}

// Classifier-free guidance with the per-channel rescale (the standard one-stage loop of the reference's scripts/generate.py:1935-1960, rescale_noise_cfg
// :688-727): the two evaluations of guided_step, then with guidance_rescale > 0 the statistics' two launches, then ONE element-wise pass.  No mask / clean:
// that loop has no conditioning.  The workspace: the partials and the statistics for the bound shape; never called while a stream is capturing
int rescaled_workspace(ltx2_dit* c) {
    const Mod& m = c->m[0];
    const int rows = channel_guidance_stats_blocks(m.N, m.Cout);
    if (c->cs_part && c->cs_rows == rows && c->cs_C == m.Cout) return LTX2_OK;
    if (c->cs_part) (void)hipFree(c->cs_part);
    c->cs_part = nullptr;
    c->cs_stats = nullptr;
    c->cs_rows = c->cs_C = 0;
    const long bytes = 8L * rows * 4 * m.Cout + 4L * 4 * m.Cout;
    if (hipMalloc((void**)&c->cs_part, bytes) != hipSuccess) {
        c->cs_part = nullptr;
        ltx2_set_error("dit_rescaled_guided_step: allocating %ld bytes of workspace failed", bytes);
        return LTX2_E_HIP;
    }
    c->cs_stats = (float*)(c->cs_part + (long)rows * 4 * m.Cout);
    c->cs_rows = rows;
    c->cs_C = m.Cout;
    return LTX2_OK;
}

int rescaled_guided_step(ltx2_dit* c, ltx2_dit* neg, const ModIn& in, const StepIo& io, float cfg_scale, double guidance_rescale, float sigma,
                         float sigma_next, hipStream_t st) {
    TRY(step_check(sigma, &io, 1, "dit_rescaled_guided_step"));
    const Mod& m = c->m[0];
    const bool rescale = guidance_rescale > 0.0;          // the reference's condition (:1930)
    LTX2_CHECK_ARG(!rescale || (c->cs_part && c->cs_rows == channel_guidance_stats_blocks(m.N, m.Cout) && c->cs_C == m.Cout),
                   "dit_rescaled_guided_step: workspace missing");
    TRY(evaluate(c, neg, &in, st));
    const long stride = in.n_ts == 1 ? 0 : 1;
    if (rescale)
        TRY(channel_guidance_stats_launch(in.latent, m.vel, neg->m[0].vel, in.ts, stride, cfg_scale, c->cs_part, c->cs_stats, m.N, m.Cout, st));
    return rescaled_guided_euler_step_launch(in.latent, m.vel, neg->m[0].vel, in.ts, stride, rescale ? c->cs_stats : nullptr, cfg_scale, guidance_rescale,
                                             sigma, sigma_next, io.latent, m.N, m.Cout, st);
}

// Spatio-temporal guidance on top (pipelines/one_stage.py:284-297): a third evaluation, on c ITSELF with the self-attentions of c->stg[0] skipped (no third
// context: its text K / V would be a second copy of c's), into the caller's scratch; then the one element-wise pass.  neg may be NULL: no CFG.
int stg_step(ltx2_dit* c, ltx2_dit* neg, const ModIn& in, const StepIo& io, float* vel_perturbed, float cfg_scale, float stg_scale, float sigma,
             float sigma_next, hipStream_t st) {
    TRY(step_check(sigma, &io, 1, "dit_stg_step"));
    LTX2_CHECK_ARG(vel_perturbed, "dit_stg_step: vel_perturbed (an [N][out_channels] fp32 scratch) is required");
    const Mod& m = c->m[0];
    TRY(evaluate(c, neg, &in, st));
    const ModIn pert[1] = {{in.latent, in.ts, in.n_ts, in.sigma, vel_perturbed}};
    TRY(forward(c, pert, st, true, true));
    return stg_euler_step_launch(in.latent, m.vel, neg ? neg->m[0].vel : nullptr, vel_perturbed, in.ts, in.n_ts == 1 ? 0 : 1, io.mask, io.clean, cfg_scale,
                                 stg_scale, sigma, sigma_next, io.latent, m.N, m.Cout, st);
}

// The same on AudioVideo contexts with BOTH latents stepped and an STG term per modality: the evaluations of guided_step_joint (neg NULL: no CFG), the
// perturbed AudioVideo forward on c itself -- the self-attentions of c->stg[0] and c->stg[1] skipped -- into the caller's scratch pair ptb, then ONE
// element-wise launch over both latents.  A modality whose stg scale is 0 hands the kernel no perturbed velocity: the guided step's arithmetic.
// (the entry has checked the scratch lengths, the sets and the scales)
int stg_step_joint(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const StepIo* io, float* const ptb[2], const float cfg[2], const float stg[2], float sigma,
                   float sigma_next, hipStream_t st) {
    TRY(step_check(sigma, io, 2, "dit_stg_step_joint_av"));
    const Mod &v = c->m[0], &a = c->m[1];
    TRY(evaluate(c, neg, in, st));
    const ModIn pert[2] = {{in[0].latent, in[0].ts, in[0].n_ts, in[0].sigma, ptb[0]}, {in[1].latent, in[1].ts, in[1].n_ts, in[1].sigma, ptb[1]}};
    TRY(forward(c, pert, st, true, true));
    return stg_euler_step_pair_launch(in[0].latent, v.vel, neg ? neg->m[0].vel : nullptr, stg[0] != 0.f ? ptb[0] : nullptr, in[0].ts, in[0].n_ts == 1 ? 0 : 1,
                                      io[0].mask, io[0].clean, cfg[0], stg[0], io[0].latent, v.N, v.Cout, in[1].latent, a.vel,
                                      neg ? neg->m[1].vel : nullptr, stg[1] != 0.f ? ptb[1] : nullptr, in[1].ts, in[1].n_ts == 1 ? 0 : 1, io[1].mask,
                                      io[1].clean, cfg[1], stg[1], io[1].latent, a.N, a.Cout, sigma, sigma_next, st);
}

// Guidance whose scalars are sums over the whole latent (CFG*, APG, legacy APG with momentum; csrc/sampler.hip): the guided step above with the
// one element-wise pass replaced by the sums kernel and the projected step kernel.
struct Projected {      // the guider of a projected step: mode 0 CFG*, 1 APG, 2 legacy APG
    int mode;
    float scale, eta, norm_threshold, momentum;
    bool running() const { return mode == 2 && momentum != 0.f; }
};

int projected_check(const Projected& g, const char* who) {
    LTX2_CHECK_ARG(g.mode >= 0 && g.mode <= 2, "%s: mode=%d is 0 (CFG*), 1 (APG) or 2 (legacy APG)", who, g.mode);
    LTX2_CHECK_ARG(g.momentum == 0.f || g.mode == 2, "%s: momentum=%g belongs to mode 2 (legacy APG) alone", who, g.momentum);
    return LTX2_OK;
}

// partials for the bound N and, with momentum, the running guidance; never called while a stream is capturing.  keep_running: the step continues a
// loop (first == 0), so a missing or differently sized running buffer is an error, not something to allocate
int projected_workspace(ltx2_dit* c, bool running, bool keep_running) {
    const Mod& m = c->m[0];
    const int rows = guidance_sums_blocks(m.N, m.Cout);
    if (!c->pg_part || c->pg_rows != rows) {
        if (c->pg_part) (void)hipFree(c->pg_part);
        c->pg_part = nullptr;
        c->pg_rows = 0;
        if (hipMalloc((void**)&c->pg_part, 8L * 5 * rows) != hipSuccess) {
            ltx2_set_error("dit_projected_step: allocating %ld bytes of workspace failed", 8L * 5 * rows);
            return LTX2_E_HIP;
        }
        c->pg_rows = rows;
    }
    const long n = (long)m.N * m.Cout;
    if (!running || (c->pg_run && c->pg_run_n == n)) return LTX2_OK;
    if (keep_running) {
        ltx2_set_error("dit_projected_step: first == 0 but no step with first != 0 has filled the running guidance for %d tokens", m.N);
        return LTX2_E_STATE;
    }
    if (c->pg_run) (void)hipFree(c->pg_run);
    c->pg_run = nullptr;
    c->pg_run_n = 0;
    if (hipMalloc((void**)&c->pg_run, 4L * n) != hipSuccess) {
        ltx2_set_error("dit_projected_step: allocating %ld bytes of workspace failed", 4L * n);
        return LTX2_E_HIP;
    }
    c->pg_run_n = n;
    return LTX2_OK;
}

int projected_step(ltx2_dit* c, ltx2_dit* neg, const ModIn& in, const StepIo& io, const Projected& g, int first, float sigma, float sigma_next, hipStream_t st) {
    TRY(step_check(sigma, &io, 1, "dit_projected_step"));
    const Mod& m = c->m[0];
    LTX2_CHECK_ARG(c->pg_part && c->pg_rows == guidance_sums_blocks(m.N, m.Cout) && (!g.running() || (c->pg_run && c->pg_run_n == (long)m.N * m.Cout)),
                   "dit_projected_step: workspace missing");
    TRY(evaluate(c, neg, &in, st));
    float* run = g.running() ? c->pg_run : nullptr;
    const long stride = in.n_ts == 1 ? 0 : 1;
    TRY(guidance_sums_launch(in.latent, m.vel, neg->m[0].vel, in.ts, stride, run, first, g.momentum, c->pg_part, m.N, m.Cout, st));
    return projected_euler_step_launch(in.latent, m.vel, neg->m[0].vel, in.ts, stride, io.mask, io.clean, run, c->pg_part, g.mode, g.scale, g.eta,
                                       g.norm_threshold, sigma, sigma_next, io.latent, nullptr, m.N, m.Cout, st);
}

// The same on AudioVideo contexts with BOTH latents stepped, each under its own guider (OneStagePipeline's joint branch with its default guiders, a
// CFGStarRescalingGuider per modality; pipelines/one_stage.py:466-568): the two evaluations of guided_step_joint, then ONE sums launch over the
// modalities whose guider reads sums and ONE step launch over both latents.  A modality's guider is one of projected_step's, plain CFG
// (PROJECTED_CFG) or none (PROJECTED_OFF).  run[k]: the caller's running guidance of a legacy APG guider with momentum, else NULL.
bool projected_sums(const Projected& g) { return g.mode < PROJECTED_CFG; }

int projected_joint_check(const Projected g[2], float* const run[2], const int64_t n_run[2], const ltx2_dit* c, const char* who) {
    for (int k = 0; k < 2; ++k) {
        LTX2_CHECK_ARG(g[k].mode >= 0 && g[k].mode <= PROJECTED_OFF, "%s: mode=%d of modality %d is 0 (CFG*), 1 (APG), 2 (legacy APG), 3 (CFG) or 4 (off)", who,
                       g[k].mode, k);
        LTX2_CHECK_ARG(g[k].momentum == 0.f || g[k].mode == 2, "%s: momentum=%g belongs to mode 2 (legacy APG) alone", who, g[k].momentum);
        // the sums kernel writes, and the step kernel reads, N * out_channels elements there on every step (the comment at cond_modality())
        const int64_t need = (int64_t)c->m[k].N * c->m[k].Cout;
        LTX2_CHECK_ARG(g[k].running() ? (run[k] && n_run[k] == need) : !run[k],
                       "%s: modality %d %s a running buffer of %d tokens x %d channels, got %ld elements", who, k,
                       g[k].running() ? "needs" : "(no momentum) takes no", c->m[k].N, c->m[k].Cout, (long)(run[k] ? n_run[k] : 0));
    }
    return LTX2_OK;
}

// each modality's partials, for the modalities whose guider reads sums; never called while a stream is capturing
int projected_joint_workspace(ltx2_dit* c, const Projected g[2]) {
    for (int k = 0; k < 2; ++k) {
        const int rows = guidance_sums_blocks(c->m[k].N, c->m[k].Cout);
        if (!projected_sums(g[k]) || (c->pgj_part[k] && c->pgj_rows[k] == rows)) continue;
        if (c->pgj_part[k]) (void)hipFree(c->pgj_part[k]);
        c->pgj_part[k] = nullptr;
        c->pgj_rows[k] = 0;
        if (hipMalloc((void**)&c->pgj_part[k], 8L * 5 * rows) != hipSuccess) {
            ltx2_set_error("dit_projected_step_joint_av: allocating %ld bytes of workspace failed", 8L * 5 * rows);
            return LTX2_E_HIP;
        }
        c->pgj_rows[k] = rows;
    }
    return LTX2_OK;
}

int projected_step_joint(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const StepIo* io, const Projected g[2], float* const run[2], int first, float sigma,
                         float sigma_next, hipStream_t st, bool rewind_events = true) {
    TRY(step_check(sigma, io, 2, "dit_projected_step_joint_av"));
    const Mod &v = c->m[0], &a = c->m[1];
    double* part[2];
    for (int k = 0; k < 2; ++k) {
        part[k] = projected_sums(g[k]) ? c->pgj_part[k] : nullptr;
        LTX2_CHECK_ARG(!projected_sums(g[k]) || (part[k] && c->pgj_rows[k] == guidance_sums_blocks(c->m[k].N, c->m[k].Cout)),
                       "dit_projected_step_joint_av: workspace missing");
    }
    TRY(evaluate(c, neg, in, st, rewind_events));
    const long stride[2] = {in[0].n_ts == 1 ? 0 : 1, in[1].n_ts == 1 ? 0 : 1};
    if (part[0] || part[1])
        TRY(guidance_sums_pair_launch(in[0].latent, v.vel, neg->m[0].vel, in[0].ts, stride[0], run[0], first, g[0].momentum, part[0], v.N, v.Cout, in[1].latent,
                                      a.vel, neg->m[1].vel, in[1].ts, stride[1], run[1], first, g[1].momentum, part[1], a.N, a.Cout, st));
    return projected_euler_step_pair_launch(in[0].latent, v.vel, neg->m[0].vel, in[0].ts, stride[0], io[0].mask, io[0].clean, run[0], part[0], g[0].mode,
                                            g[0].scale, g[0].eta, g[0].norm_threshold, io[0].latent, nullptr, v.N, v.Cout, in[1].latent, a.vel,
                                            neg->m[1].vel, in[1].ts, stride[1], io[1].mask, io[1].clean, run[1], part[1], g[1].mode, g[1].scale, g[1].eta,
                                            g[1].norm_threshold, io[1].latent, nullptr, a.N, a.Cout, sigma, sigma_next, st);
}

// Multi-modal guidance on AudioVideo contexts (the reference's two-stage pipeline, pipelines/two_stage.py:314-401; MultiModalGuider.calculate): per step
// up to four evaluations of BOTH modalities -- c, neg (NULL: no CFG term), c with the self-attentions of c->stg skipped into the caller's ptb scratch
// (NULL: no STG term), c with every cross-modal attention skipped into the caller's mod scratch (NULL: no modality term) -- and then both latents stepped,
// each modality under its own scales.  Without rescale that is ONE launch over both latents; a modality with rescale takes its sums and its step launch.
struct MmGuide {        // one modality's MultiModalGuiderParams
    float cfg, stg, mod, rescale;
};

// each modality's partials, for the modalities that rescale; never called while a stream is capturing
int mm_workspace(ltx2_dit* c, const MmGuide g[2]) {
    for (int k = 0; k < 2; ++k) {
        const int rows = guidance_sums_blocks(c->m[k].N, c->m[k].Cout);
        if (g[k].rescale == 0.f || (c->mm_part[k] && c->mm_rows[k] == rows)) continue;
        if (c->mm_part[k]) (void)hipFree(c->mm_part[k]);
        c->mm_part[k] = nullptr;
        c->mm_rows[k] = 0;
        if (hipMalloc((void**)&c->mm_part[k], 8L * 4 * rows) != hipSuccess) {
            ltx2_set_error("dit_mm_guided_step_av: allocating %ld bytes of workspace failed", 8L * 4 * rows);
            return LTX2_E_HIP;
        }
        c->mm_rows[k] = rows;
    }
    return LTX2_OK;
}

int mm_guided_step(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const StepIo* io, float* const mod[2], float* const ptb[2], const MmGuide g[2], float sigma,
                   float sigma_next, hipStream_t st) {
    for (int k = 0; k < 2; ++k)      // (the entry has checked the scalars, the conditionings and the scratch buffers)
        LTX2_CHECK_ARG(g[k].rescale == 0.f || (c->mm_part[k] && c->mm_rows[k] == guidance_sums_blocks(c->m[k].N, c->m[k].Cout)),
                       "dit_mm_guided_step_av: workspace missing");
    TRY(evaluate(c, neg, in, st));
    if (ptb[0]) {
        const ModIn p[2] = {{in[0].latent, in[0].ts, in[0].n_ts, in[0].sigma, ptb[0]}, {in[1].latent, in[1].ts, in[1].n_ts, in[1].sigma, ptb[1]}};
        TRY(forward(c, p, st, true, true));
    }
    if (mod[0]) {
        const ModIn q[2] = {{in[0].latent, in[0].ts, in[0].n_ts, in[0].sigma, mod[0]}, {in[1].latent, in[1].ts, in[1].n_ts, in[1].sigma, mod[1]}};
        TRY(forward(c, q, st, true, false, true));
    }
    const Mod* m[2] = {&c->m[0], &c->m[1]};
    const float* vu[2] = {neg ? neg->m[0].vel : nullptr, neg ? neg->m[1].vel : nullptr};
    const long stride[2] = {in[0].n_ts == 1 ? 0 : 1, in[1].n_ts == 1 ? 0 : 1};
    if (g[0].rescale == 0.f && g[1].rescale == 0.f)
        return mm_guided_euler_step_pair_launch(in[0].latent, m[0]->vel, vu[0], ptb[0], mod[0], in[0].ts, stride[0], io[0].mask, io[0].clean, g[0].cfg, g[0].stg,
                                                g[0].mod, io[0].latent, m[0]->N, m[0]->Cout, in[1].latent, m[1]->vel, vu[1], ptb[1], mod[1], in[1].ts, stride[1],
                                                io[1].mask, io[1].clean, g[1].cfg, g[1].stg, g[1].mod, io[1].latent, m[1]->N, m[1]->Cout, sigma, sigma_next, st);
    for (int k = 0; k < 2; ++k) {
        if (g[k].rescale == 0.f) {
            TRY(mm_guided_euler_step_launch(in[k].latent, m[k]->vel, vu[k], ptb[k], mod[k], in[k].ts, stride[k], io[k].mask, io[k].clean, g[k].cfg, g[k].stg,
                                            g[k].mod, sigma, sigma_next, io[k].latent, m[k]->N, m[k]->Cout, st));
            continue;
        }
        TRY(mm_guidance_sums_launch(in[k].latent, m[k]->vel, vu[k], ptb[k], mod[k], in[k].ts, stride[k], g[k].cfg, g[k].stg, g[k].mod, c->mm_part[k], nullptr,
                                    m[k]->N, m[k]->Cout, st));
        TRY(mm_rescaled_euler_step_launch(in[k].latent, m[k]->vel, vu[k], ptb[k], mod[k], in[k].ts, stride[k], io[k].mask, io[k].clean, c->mm_part[k], g[k].cfg,
                                          g[k].stg, g[k].mod, g[k].rescale, sigma, sigma_next, io[k].latent, nullptr, m[k]->N, m[k]->Cout, st));
    }
    return LTX2_OK;
}

// The res_2s second-order step (reference pipelines/ti2vid_hq.py:153-319; HQ pipeline stage 1): per step two pairs of evaluations, the second
// from a midpoint latent at the geometric-mean sub-sigma, and two element-wise passes.  On AudioVideo contexts the JOINT step: both latents are stepped,
// the video under cfg_scale and the audio under audio_cfg_scale, each pass one launch over both.
// phi_j(z) and the res_2s coefficients exactly as components/res2s.py computes them, in double
double res2s_phi(int j, double z) {
    double fact = 1;
    for (int k = 2; k <= j; ++k) fact *= k;
    if (std::fabs(z) < 1e-10) return 1.0 / fact;
    double rem = 0, kf = 1;
    for (int k = 0; k < j; ++k) {
        if (k > 0) kf *= k;
        rem += std::pow(z, k) / kf;
    }
    return (std::exp(z) - rem) / std::pow(z, j);
}

struct Res2sPlan {      // what one step does, decided on the host from (sigma, sigma_next)
    bool last;          // the final-step branch: latent = d
    float c, h, b1, b2, sub_sigma;
    int n_bong;
};

int res2s_plan(float sigma_f, float sigma_next_f, Res2sPlan& p) {
    LTX2_CHECK_ARG(sigma_f > 0.f && sigma_next_f >= 0.f, "dit_res2s_step: sigma=%g must be > 0 and sigma_next=%g >= 0", sigma_f, sigma_next_f);
    const double sigma = sigma_f, sigma_next = sigma_next_f, c2 = 0.5;
    const double h = sigma_next > 0 ? -std::log(sigma_next / sigma) : 0.0;
    p = Res2sPlan{h == 0.0 || sigma_next <= 0.001, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
    if (p.last) return LTX2_OK;
    const double a21 = c2 * res2s_phi(1, -h * c2), b2 = res2s_phi(2, -h) / c2, b1 = res2s_phi(1, -h) - b2;
    p.c = (float)(h * a21);
    p.h = (float)h;
    p.b1 = (float)b1;
    p.b2 = (float)b2;
    p.sub_sigma = (float)std::sqrt(sigma * sigma_next);
    p.n_bong = (h < 0.5 && sigma > 0.03) ? 100 : 0;
    return LTX2_OK;
}

// three fp32 buffers per modality, x_mid | anchor | eps1 of res2s_each(c, k) elements, the video's then the audio's (such a context has no other use for
// the workspace); r2s_each is res2s_total(c).  Never called while a stream is capturing
int res2s_workspace(ltx2_dit* c, long each) {
    if (c->r2s && c->r2s_each == each) return LTX2_OK;
    if (c->r2s) (void)hipFree(c->r2s);
    c->r2s = nullptr;
    c->r2s_each = 0;
    if (hipMalloc((void**)&c->r2s, 4L * 3 * each) != hipSuccess) {
        ltx2_set_error("dit_res2s_step: allocating %ld bytes of workspace failed", 4L * 3 * each);
        return LTX2_E_HIP;
    }
    c->r2s_each = each;
    return LTX2_OK;
}
long res2s_each(const ltx2_dit* c, int k) { return align_up((long)c->m[k].N * c->m[k].Cout, 64); }
long res2s_total(const ltx2_dit* c) { return res2s_each(c, 0) + (c->av ? res2s_each(c, 1) : 0); }

// in[k]: (latent, timesteps, sigma) of modality k; v_ts_sub / a_ts_sub / sub_sigma: the same at the sub-sigma.  cond_sub: in a captured conditioned
// loop, the masks from which ts_sub = mask * sub_sigma is formed into the buffer `in[k].ts` points at, after the midpoint kernel has read it (one
// stream, in order).  Every check stands before the first launch.
int res2s_step(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const float* v_ts_sub, const float* a_ts_sub, const float* sub_sigma, const Cond* cond_sub,
               const StepIo* io, float cfg_scale, float audio_cfg_scale, const Res2sPlan& p, hipStream_t st) {
    const int nm = c->av ? 2 : 1;
    const float cfg[2] = {cfg_scale, audio_cfg_scale};
    const float *ts_sub[2] = {v_ts_sub, a_ts_sub}, *vu[2] = {};
    float *x_mid[2] = {}, *anchor[2] = {}, *eps1[2] = {};
    long stride[2] = {};
    LTX2_CHECK_ARG(c->r2s && c->r2s_each == res2s_total(c), "dit_res2s_step: workspace missing");
    float* base = c->r2s;
    for (int k = 0; k < nm; ++k) {
        LTX2_CHECK_ARG((io[k].mask == nullptr) == (io[k].clean == nullptr), "dit_res2s_step: mask and clean go together");
        if (cond_sub && cond_sub[k].mask) ts_sub[k] = c->m[k].ts_tok;
        LTX2_CHECK_ARG(p.last || (sub_sigma && ts_sub[k]), "dit_res2s_step: the sub-sigma timesteps are missing");
        const long each = res2s_each(c, k);
        x_mid[k] = p.last ? io[k].latent : base;                // the final step (p.c == 0, p.n_bong == 0): latent = d, nothing kept
        anchor[k] = p.last ? nullptr : base + each;
        eps1[k] = p.last ? nullptr : base + 2 * each;
        base += 3 * each;
        vu[k] = neg ? neg->m[k].vel : nullptr;
        stride[k] = in[k].n_ts == 1 ? 0 : 1;
    }
    const Mod &v = c->m[0], &a = c->m[1];
    TRY(evaluate(c, neg, in, st));
    if (nm == 1)
        TRY(res2s_midpoint_launch(in[0].latent, v.vel, vu[0], in[0].ts, stride[0], io[0].mask, io[0].clean, cfg[0], p.c, p.n_bong, x_mid[0], anchor[0], eps1[0],
                                  v.N, v.Cout, st));
    else
        TRY(res2s_midpoint_pair_launch(in[0].latent, v.vel, vu[0], in[0].ts, stride[0], io[0].mask, io[0].clean, cfg[0], x_mid[0], anchor[0], eps1[0], v.N, v.Cout,
                                       in[1].latent, a.vel, vu[1], in[1].ts, stride[1], io[1].mask, io[1].clean, cfg[1], x_mid[1], anchor[1], eps1[1], a.N, a.Cout,
                                       p.c, p.n_bong, st));
    if (p.last) return LTX2_OK;
    ModIn mid[2] = {};
    for (int k = 0; k < nm; ++k) {
        if (cond_sub && cond_sub[k].mask) {
            hipLaunchKernelGGL(mask_sigma_kernel, dim3((c->m[k].N + 255) / 256), dim3(256), 0, st, cond_sub[k].mask, sub_sigma, c->m[k].ts_tok, c->m[k].N);
            LTX2_CHECK_LAUNCH("mask_sigma_kernel");
        }
        mid[k] = {x_mid[k], ts_sub[k], in[k].n_ts, sub_sigma, nullptr};
    }
    TRY(evaluate(c, neg, mid, st));
    if (nm == 1)
        return res2s_combine_launch(x_mid[0], v.vel, vu[0], ts_sub[0], stride[0], io[0].mask, io[0].clean, cfg[0], anchor[0], eps1[0], p.h, p.b1, p.b2, io[0].latent,
                                    v.N, v.Cout, st);
    return res2s_combine_pair_launch(x_mid[0], v.vel, vu[0], ts_sub[0], stride[0], io[0].mask, io[0].clean, cfg[0], anchor[0], eps1[0], io[0].latent, v.N, v.Cout,
                                     x_mid[1], a.vel, vu[1], ts_sub[1], stride[1], io[1].mask, io[1].clean, cfg[1], anchor[1], eps1[1], io[1].latent, a.N, a.Cout,
                                     p.h, p.b1, p.b2, st);
}

// The Heun sampler and the GE velocity correction of OneStagePipeline (reference pipelines/one_stage.py:300-307, 334-464, 570-729) under a plain CFGGuider
// or none.  Heun: per step two pairs of evaluations, the second from the Euler predictor xp at sigma_next, and two element-wise passes; when sigma_next == 0
// one pair and latent = d.  On AudioVideo contexts the JOINT step, each pass one launch over both latents.  GE (ge_gamma > 0) corrects the VIDEO's guided
// x0 of the first evaluation from the previous step's velocity, kept in the workspace.
// The workspace: the video's prev | d | xp, then on an AudioVideo context the audio's d | xp, each of heun_each(c, k) elements.  keep_prev: the step
// continues a GE loop (first == 0), so it is an error unless a step entry with GE and first != 0 has filled prev in this very workspace (a step
// without GE, or a capture, allocates it and leaves prev unfilled).  Never called while a stream is capturing
long heun_each(const ltx2_dit* c, int k) { return align_up((long)c->m[k].N * c->m[k].Cout, 64); }
long heun_total(const ltx2_dit* c) { return 3 * heun_each(c, 0) + (c->av ? 2 * heun_each(c, 1) : 0); }

int heun_workspace(ltx2_dit* c, bool keep_prev) {
    const long n = heun_total(c);
    const bool have = c->heun && c->heun_n == n;
    if (keep_prev && !(have && c->heun_prev)) {
        ltx2_set_error("dit_heun_step: first == 0 but no step with first != 0 has filled the GE velocity for %d tokens", c->m[0].N);
        return LTX2_E_STATE;
    }
    if (have) return LTX2_OK;
    if (c->heun) (void)hipFree(c->heun);
    c->heun = nullptr;
    c->heun_n = 0;
    c->heun_prev = false;
    if (hipMalloc((void**)&c->heun, 4L * n) != hipSuccess) {
        ltx2_set_error("dit_heun_step: allocating %ld bytes of workspace failed", 4L * n);
        return LTX2_E_HIP;
    }
    c->heun_n = n;
    return LTX2_OK;
}

int heun_check(const ltx2_dit* c, const StepIo* io, float ge_gamma, float sigma, float sigma_next, const char* who) {
    LTX2_CHECK_ARG(sigma > 0.f && sigma_next >= 0.f, "%s: sigma=%g must be > 0 and sigma_next=%g >= 0", who, sigma, sigma_next);
    LTX2_CHECK_ARG(ge_gamma >= 0.f, "%s: ge_gamma=%g must be >= 0 (0: no GE)", who, ge_gamma);
    for (int k = 0; k < (c->av ? 2 : 1); ++k) LTX2_CHECK_ARG((io[k].mask == nullptr) == (io[k].clean == nullptr), "%s: mask and clean go together", who);
    return LTX2_OK;
}

// in[k]: (latent, timesteps, sigma) of modality k; ts_next / sigma_next_dev: the same at sigma_next.  cond_next: in a captured conditioned loop, the masks
// from which mask * sigma_next is formed into the buffer `in[k].ts` points at, after the predictor has read it (one stream, in order).  Every check
// stands before the first launch.
int heun_step(ltx2_dit* c, ltx2_dit* neg, const ModIn* in, const float* const ts_next_in[2], const float* sigma_next_dev, const Cond* cond_next,
              const StepIo* io, const float cfg[2], float ge_gamma, int first, float sigma, float sigma_next, hipStream_t st) {
    const int nm = c->av ? 2 : 1;
    const bool last = sigma_next == 0.f;
    TRY(heun_check(c, io, ge_gamma, sigma, sigma_next, "dit_heun_step"));
    LTX2_CHECK_ARG(c->heun && c->heun_n == heun_total(c), "dit_heun_step: workspace missing");
    float* const prev = ge_gamma > 0.f ? c->heun : nullptr;
    float* d[2] = {c->heun + heun_each(c, 0), c->heun + 3 * heun_each(c, 0)};
    float* xp[2] = {d[0] + heun_each(c, 0), d[1] + (c->av ? heun_each(c, 1) : 0)};
    const float *ts_next[2] = {ts_next_in[0], ts_next_in[1]}, *vu[2] = {};
    long stride[2] = {};
    for (int k = 0; k < nm; ++k) {
        if (cond_next && cond_next[k].mask) ts_next[k] = c->m[k].ts_tok;
        LTX2_CHECK_ARG(last || (sigma_next_dev && ts_next[k]), "dit_heun_step: the timesteps of sigma_next are missing");
        vu[k] = neg ? neg->m[k].vel : nullptr;
        stride[k] = in[k].n_ts == 1 ? 0 : 1;
        if (last) {                                         // the step ends with latent = d
            d[k] = io[k].latent;
            xp[k] = nullptr;
        }
    }
    const Mod &v = c->m[0], &a = c->m[1];
    TRY(evaluate(c, neg, in, st));
    if (nm == 1)
        TRY(heun_predict_launch(in[0].latent, v.vel, vu[0], in[0].ts, stride[0], io[0].mask, io[0].clean, cfg[0], ge_gamma, prev, first, sigma, sigma_next, d[0],
                                xp[0], v.N, v.Cout, st));
    else
        TRY(heun_predict_pair_launch(in[0].latent, v.vel, vu[0], in[0].ts, stride[0], io[0].mask, io[0].clean, cfg[0], ge_gamma, prev, first, d[0], xp[0], v.N,
                                     v.Cout, in[1].latent, a.vel, vu[1], in[1].ts, stride[1], io[1].mask, io[1].clean, cfg[1], d[1], xp[1], a.N, a.Cout, sigma,
                                     sigma_next, st));
    if (last) return LTX2_OK;
    ModIn at_next[2] = {};
    for (int k = 0; k < nm; ++k) {
        if (cond_next && cond_next[k].mask) {
            hipLaunchKernelGGL(mask_sigma_kernel, dim3((c->m[k].N + 255) / 256), dim3(256), 0, st, cond_next[k].mask, sigma_next_dev, c->m[k].ts_tok, c->m[k].N);
            LTX2_CHECK_LAUNCH("mask_sigma_kernel");
        }
        at_next[k] = {xp[k], ts_next[k], in[k].n_ts, sigma_next_dev, nullptr};
    }
    TRY(evaluate(c, neg, at_next, st));
    if (nm == 1)
        return heun_correct_launch(in[0].latent, d[0], xp[0], v.vel, vu[0], ts_next[0], stride[0], io[0].mask, io[0].clean, cfg[0], sigma, sigma_next, io[0].latent,
                                   v.N, v.Cout, st);
    return heun_correct_pair_launch(in[0].latent, d[0], xp[0], v.vel, vu[0], ts_next[0], stride[0], io[0].mask, io[0].clean, cfg[0], io[0].latent, v.N, v.Cout,
                                    in[1].latent, d[1], xp[1], a.vel, vu[1], ts_next[1], stride[1], io[1].mask, io[1].clean, cfg[1], io[1].latent, a.N, a.Cout,
                                    sigma, sigma_next, st);
}

// The Euler step with GE on VideoOnly contexts (:267-326): the evaluations of guided_step (neg NULL: one), then ONE element-wise pass
int ge_step(ltx2_dit* c, ltx2_dit* neg, const ModIn& in, const StepIo& io, float cfg_scale, float ge_gamma, int first, float sigma, float sigma_next,
            hipStream_t st) {
    TRY(heun_check(c, &io, ge_gamma, sigma, sigma_next, "dit_ge_step"));
    LTX2_CHECK_ARG(ge_gamma > 0.f, "dit_ge_step: ge_gamma=%g must be > 0 (without GE the step is ltx2_dit_guided_step or ltx2_dit_denoise_step)", ge_gamma);
    LTX2_CHECK_ARG(c->heun && c->heun_n == heun_total(c), "dit_ge_step: workspace missing");
    const Mod& m = c->m[0];
    TRY(evaluate(c, neg, &in, st));
    return ge_euler_step_launch(in.latent, m.vel, neg ? neg->m[0].vel : nullptr, in.ts, in.n_ts == 1 ? 0 : 1, io.mask, io.clean, cfg_scale, ge_gamma, c->heun, first,
                                sigma, sigma_next, io.latent, m.N, m.Cout, st);
}

// The one captured sampling loop behind every ltx2_dit_graph_capture* entry: per step, sigma_i read on the device, each modality's timesteps (sigma_i, or
// mask * sigma_i where it is conditioned), then the step that LoopStep names.  All but the plain step run on VideoOnly contexts (latent[0] / cond[0]
// only), form ts = mask * sigma_i in c's buffer and let both contexts read it; the guided step on AudioVideo contexts steps latent[0] alone and reads
// latent[1] (cond[1]: its mask, for the timesteps only), unless it is the joint one, which steps and blends both.  The event pool is rewound on step 0 only, so no event is re-recorded
// inside the capture.
struct LoopStep {                           // all defaults: the plain denoise step
    ltx2_dit* neg = nullptr;                // the negative prompt's context: a guided step, or guidance inside the two below
    float cfg_scale = 0.f;
    const Projected* projected = nullptr;   // the projected step with this guider
    const Res2sPlan* res2s = nullptr;       // the res_2s step: one plan per step
    float* stg_vel = nullptr;               // the STG step into this scratch on the first stg_steps steps, then the guided (neg) or the plain step
    float stg_scale = 0.f;
    int stg_steps = 0;
    bool joint = false;                     // the guided step on AudioVideo contexts steps BOTH latents, the audio one under audio_cfg_scale
    float audio_cfg_scale = 0.f;
    const Projected* projected_joint = nullptr;     // with joint: each modality under its own guider, [2]
    float* const* running_joint = nullptr;          //   and its running guidance, [2] (NULL where the guider keeps none)
    bool heun = false;                      // the Heun step under cfg_scale (neg NULL: not guided), with GE where ge_gamma > 0
    float ge_gamma = 0.f;
    bool rescaled = false;                  // the guided step of the standard one-stage loop: CFG in its order, the per-channel rescale at guidance_rescale > 0
    double guidance_rescale = 0.0;
    const float* ancestral_up = nullptr;    // the Euler-ancestral step (neg NULL: not guided; on AudioVideo contexts over both latents, with `joint`):
    const float* ancestral_down = nullptr;  //   sigma_up / sigma_down per step (host), and the seed word (device), which stays a pointer in the graph
    const uint64_t* ancestral_seed = nullptr;
};

int capture_loop(ltx2_dit* c, const LoopStep& step, float* const latent[2], const Cond cond[2], const float* host_sigmas, int n_steps, hipStream_t st) {
    const int nm = c->av ? 2 : 1;
    float sub[64];
    for (int i = 0; step.res2s && i < n_steps; ++i) sub[i] = step.res2s[i].sub_sigma;
    TRY(begin_capture(c, host_sigmas, n_steps, st, step.res2s ? sub : nullptr));
    int rc = LTX2_OK;
    // the head of the chain: every replay starts from a cleared running guidance
    if (step.projected && step.projected->running() && hipMemsetAsync(c->pg_run, 0, 4L * c->pg_run_n, st) != hipSuccess) {
        ltx2_set_error("dit_graph_capture_projected: hipMemsetAsync failed");
        rc = LTX2_E_HIP;
    }
    for (int k = 0; step.projected_joint && k < 2 && rc == LTX2_OK; ++k)
        if (step.projected_joint[k].running() && hipMemsetAsync(step.running_joint[k], 0, 4L * c->m[k].N * c->m[k].Cout, st) != hipSuccess) {
            ltx2_set_error("dit_graph_capture_projected_joint_av: hipMemsetAsync failed");
            rc = LTX2_E_HIP;
        }
    if (step.heun && step.ge_gamma > 0.f && rc == LTX2_OK && hipMemsetAsync(c->heun, 0, 4L * heun_each(c, 0), st) != hipSuccess) {     // the GE velocity
        ltx2_set_error("dit_graph_capture_heun: hipMemsetAsync failed");
        rc = LTX2_E_HIP;
    }
    for (int i = 0; i < n_steps && rc == LTX2_OK; ++i) {
        const float *s = c->sigmas_dev + i, *ss = c->sigmas_dev + 64 + i;
        const float sigma = host_sigmas[i], sigma_next = host_sigmas[i + 1];
        ModIn in[2];
        StepIo io[2];
        for (int k = 0; k < nm && rc == LTX2_OK; ++k) {
            in[k] = {latent[k], s, 1, s, nullptr};
            io[k] = {latent[k], nullptr, nullptr, nullptr};
            rc = cond_modality(c, k, cond[k], s, in[k], io[k], st, !(step.neg && c->av && k == 1 && !step.joint));
        }
        if (rc != LTX2_OK) break;
        if (step.res2s) {
            rc = res2s_step(c, step.neg, in, ss, ss, ss, cond, io, step.cfg_scale, step.cfg_scale, step.res2s[i], st);
            if (step.res2s[i].last) break;                      // the reference's loop ends on its final step
        } else if (step.heun) {                                 // sigma_{i+1} follows sigma_i on the device; the final-step form where it is 0
            const float* const next[2] = {s + 1, s + 1};
            const float cfg[2] = {step.cfg_scale, step.cfg_scale};
            rc = heun_step(c, step.neg, in, next, s + 1, cond, io, cfg, step.ge_gamma, i == 0, sigma, sigma_next, st);
        } else if (step.ancestral_up) {
            const float cfg[2] = {step.cfg_scale, step.audio_cfg_scale};
            rc = ancestral_step(c, step.neg, in, io, cfg, sigma, {step.ancestral_up[i], step.ancestral_down[i], step.ancestral_seed, (uint32_t)i}, st, i == 0);
        } else if (step.rescaled) {
            rc = rescaled_guided_step(c, step.neg, in[0], io[0], step.cfg_scale, step.guidance_rescale, sigma, sigma_next, st);
        } else if (step.projected) {
            rc = projected_step(c, step.neg, in[0], io[0], *step.projected, i == 0, sigma, sigma_next, st);
        } else if (step.stg_vel && i < step.stg_steps) {
            rc = stg_step(c, step.neg, in[0], io[0], step.stg_vel, step.cfg_scale, step.stg_scale, sigma, sigma_next, st);
        } else if (step.projected_joint) {
            rc = projected_step_joint(c, step.neg, in, io, step.projected_joint, step.running_joint, i == 0, sigma, sigma_next, st, i == 0);
        } else if (step.neg && step.joint) {
            const float cfg[2] = {step.cfg_scale, step.audio_cfg_scale};
            rc = guided_step_joint(c, step.neg, in, io, cfg, sigma, sigma_next, st, i == 0);
        } else if (step.neg && c->av) {
            rc = guided_step(c, step.neg, in, io[0], step.cfg_scale, sigma, sigma_next, st, i == 0);
        } else if (step.neg) {
            rc = guided_step(c, step.neg, in, io[0], step.cfg_scale, sigma, sigma_next, st, i == 0);
        } else {
            rc = denoise_step(c, in, io, sigma, sigma_next, st, i == 0);
        }
    }
    return end_capture(c, rc, st);
}

// The latents and the conditioning of a guided capture entry's loop, and what each such entry checks first
struct LoopIo {
    float* lat[2];
    Cond cond[2];
};

// joint: both latents are stepped, so the audio's mask and clean latent go together as the video's do (otherwise the audio's mask gives timesteps only)
int capture_ready(ltx2_dit* c, ltx2_dit* neg, bool need_neg, bool want_av, const LoopIo& lo, const float* host_sigmas, int n_steps, const char* who,
                  bool joint = false) {
    LTX2_CHECK_ARG(c && lo.lat[0] && (!want_av || lo.lat[1]) && host_sigmas && n_steps > 0 && n_steps < 64, "%s: bad argument", who);
    LTX2_CHECK_ARG(neg || !need_neg, "%s: null context", who);
    const int n_ts[2] = {lo.cond[0].mask ? c->m[0].N : 1, lo.cond[1].mask ? c->m[1].N : 1};
    TRY(step_ready(c, neg, want_av, n_ts, who));
    for (int k = 0; k < (joint ? 2 : 1); ++k)
        LTX2_CHECK_ARG((lo.cond[k].mask == nullptr) == (lo.cond[k].clean == nullptr), "%s: mask and clean go together", who);
    return LTX2_OK;
}
}  // namespace

namespace {
// ---------------------------------- first-block cache (VideoOnly contexts, opt-in) ----------------------------------
// Everything of it is below this line: with the cache off no line of it runs, and forward() and every other entry are what they were.
// A slot: one kind of evaluation within a step (the positive or the negative pass).
struct FbcSlot {
    float *head_prev = nullptr, *tail = nullptr;
    bool valid = false, force = false;      // force: the next evaluation computes whatever the metric says (consumed by it)
    int64_t evals = 0, skips = 0;
    double num = 0.0, den = 0.0;            // the last metric read back (an evaluation that was forced, or had no valid state, reads none)
};
// A context's cache, kept beside the context (fbc_states) so that ltx2_dit itself is unchanged: per slot head_prev | tail, then the shared scratch r
// and the saved h1, each [N][D] fp32, then the metric's partials and its record -- ONE allocation, made on first use for the bound shape and
// freed by ltx2_dit_fbc_configure(ctx, 0, 0), which a caller issues before ltx2_dit_destroy.  A pass through another context (the negative
// prompt's) uses the slots of the context the step was called on.
struct FbcState {
    int D = 0;
    std::vector<FbcSlot> fbc_slots;
    float fbc_threshold = 0.f;
    float* fbc_buf = nullptr;
    long fbc_n = 0;                    //   elements of each buffer the allocation was made for
    float *fbc_r = nullptr, *fbc_save = nullptr;
    double* fbc_part = nullptr;
    FbcRecord* fbc_rec = nullptr;
    FbcRecord* fbc_host = nullptr;     //   pinned: where the step's stream copies the record for the host's decision
};
std::unordered_map<const ltx2_dit*, FbcState> fbc_states;
FbcState* fbc_state(const ltx2_dit* c) {
    auto it = fbc_states.find(c);
    return it == fbc_states.end() ? nullptr : &it->second;
}

// The cut between layer 0 and layer 1.  h0 is copied aside in front of layer 0 (the blocks update the stream in place); behind it fbc_head_metric
// forms r = h1 - h0, the sums against the slot's head_prev and the decision, and overwrites the saved h0 with h1.  The record comes back by one
// 24-byte copy on `st` and a wait for it -- the pass is eager, never captured.  A skip adds the slot's tail to the stream and leaves the loop;
// otherwise layers 1..L-1 run, tail = hL - h1 is stored and r becomes head_prev by a pointer swap.
struct FbcPass {
    FbcState* owner;        // the state of the context that holds the slots (c itself, or the positive context of a guided step)
    int slot;
};

int fbc_workspace(FbcState* o, long n) {
    if (o->fbc_buf && o->fbc_n == n) return LTX2_OK;
    if (o->fbc_buf) (void)hipFree(o->fbc_buf);
    o->fbc_buf = nullptr;
    o->fbc_n = 0;
    const long slots = (long)o->fbc_slots.size(), each = align_up(4L * n), nb = fbc_metric_blocks(n);
    const long bytes = (2 * slots + 2) * each + align_up(16L * nb) + align_up((long)sizeof(FbcRecord));
    if (hipMalloc((void**)&o->fbc_buf, bytes) != hipSuccess) {
        o->fbc_buf = nullptr;
        ltx2_set_error("dit_fbc: allocating %ld bytes of cache buffers failed", bytes);
        return LTX2_E_HIP;
    }
    if (!o->fbc_host && hipHostMalloc((void**)&o->fbc_host, sizeof(FbcRecord)) != hipSuccess) {
        o->fbc_host = nullptr;
        ltx2_set_error("dit_fbc: allocating the pinned record failed");
        return LTX2_E_HIP;
    }
    char* p = (char*)o->fbc_buf;
    for (FbcSlot& s : o->fbc_slots) {
        s.head_prev = (float*)p;
        s.tail = (float*)(p + each);
        s.valid = false;            // the buffers are new: nothing to compare with
        p += 2 * each;
    }
    o->fbc_r = (float*)p;
    o->fbc_save = (float*)(p + each);
    o->fbc_part = (double*)(p + 2 * each);
    o->fbc_rec = (FbcRecord*)(p + 2 * each + align_up(16L * nb));
    o->fbc_n = n;
    return LTX2_OK;
}

// everything a cached pass refuses, before anything is enqueued; allocates the buffers for c's bound shape
int fbc_ready(ltx2_dit* c, const FbcPass& f, hipStream_t st, const char* who) {
    FbcState* o = f.owner;
    if (c->av) {
        ltx2_set_error("%s: the first-block cache is built for the VideoOnly model alone (AudioVideo contexts are not)", who);
        return LTX2_E_UNSUPPORTED;
    }
    LTX2_CHECK_ARG(o && !o->fbc_slots.empty(), "%s: the first-block cache is off (ltx2_dit_fbc_configure)", who);
    LTX2_CHECK_ARG(f.slot >= 0 && f.slot < (int)o->fbc_slots.size(), "%s: slot=%d, %d configured", who, f.slot, (int)o->fbc_slots.size());
    LTX2_CHECK_ARG(c->cfg.num_layers >= 2 && c->m[0].D == o->D, "%s: the model needs 2 layers at least, and one width in both contexts", who);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        ltx2_set_error("%s: a cached pass reads its decision back on the host and cannot be captured into a graph", who);
        return LTX2_E_STATE;
    }
    return fbc_workspace(o, (long)c->m[0].N * c->m[0].D);
}

int fbc_before_head(ltx2_dit* c, const FbcPass& f, hipStream_t st) {
    const Mod& m = c->m[0];
    if (hipMemcpyAsync(f.owner->fbc_save, m.x, 4L * m.N * m.D, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        ltx2_set_error("dit_fbc: saving the residual stream failed");
        return LTX2_E_HIP;
    }
    return LTX2_OK;
}

int fbc_after_head(ltx2_dit* c, const FbcPass& f, hipStream_t st, bool& skip) {
    FbcState* o = f.owner;
    FbcSlot& s = o->fbc_slots[f.slot];
    const Mod& m = c->m[0];
    const long n = (long)m.N * m.D;
    skip = false;
    TRY(fbc_head_metric_launch(o->fbc_save, m.x, s.valid ? s.head_prev : nullptr, o->fbc_r, o->fbc_save, o->fbc_part, o->fbc_rec, o->fbc_threshold, n, st));
    const bool forced = s.force;
    s.force = false;
    s.evals += 1;
    if (!s.valid || forced) return LTX2_OK;
    if (hipMemcpyAsync(o->fbc_host, o->fbc_rec, sizeof(FbcRecord), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        ltx2_set_error("dit_fbc: reading the decision back failed");
        return LTX2_E_HIP;
    }
    s.num = o->fbc_host->num;
    s.den = o->fbc_host->den;
    if (o->fbc_host->skip == 0) return LTX2_OK;
    TRY(fbc_apply_tail_launch(m.x, s.tail, n, st));
    s.skips += 1;
    skip = true;
    return LTX2_OK;
}

int fbc_after_tail(ltx2_dit* c, const FbcPass& f, hipStream_t st) {
    FbcState* o = f.owner;
    FbcSlot& s = o->fbc_slots[f.slot];
    const Mod& m = c->m[0];
    TRY(fbc_store_tail_launch(m.x, o->fbc_save, s.tail, (long)m.N * m.D, st));
    std::swap(s.head_prev, o->fbc_r);           // r becomes head_prev; the old head_prev is the next scratch
    s.valid = true;
    return LTX2_OK;
}

// forward() for one VideoOnly modality and a plain pass, cut behind layer 0: the same launches in the same order, with the cache's three steps
// around layer 0 and behind the last layer.  Every refusal stands before anything is enqueued.
int forward_fbc(ltx2_dit* c, const ModIn* in, hipStream_t st, const FbcPass& f, const char* who) {
    TRY(fbc_ready(c, f, st, who));
    c->sync_next = 0;
    Mod& m = c->m[0];
    const ModW& w = c->mw[0];
    LTX2_CHECK_ARG(in[0].n_ts == 1 || in[0].n_ts == m.N, "%s: n_timesteps=%d must be 1 or N=%d", who, in[0].n_ts, m.N);
    LTX2_CHECK_ARG(in[0].n_ts == 1 || c->per_token, "%s: workspace was not sized for per-token timesteps", who);
    long es = 0, ee = 0;
    TRY(cast_f32_bf16_launch(in[0].latent, m.lat, (long)m.N * m.Cin, st));
    TRY(dense(c, gemm_dense_params(m.lat, m.Cin, w.patch_w, w.patch_b, m.x, m.D, m.N, m.D, m.Cin), EPI_F32, st));
    TRY(adaln_chain(c, m, w.ada, in[0].ts, 1, in[0].n_ts, c->cfg.timestep_scale, m.emb, m.e_f, st));
    if (in[0].n_ts > 1) {
        es = (long)w.ada.rows * m.D;
        ee = m.D;
    } else if (c->adaln_combine) {
        TRY(adaln_combine_launch(m.sst_all, m.emb, m.comb, c->cfg.num_layers, (long)w.ada.rows * m.D, st));
    }
    m.use_comb = in[0].n_ts == 1 && c->adaln_combine;
    if (c->v2) TRY(adaln_chain(c, m, w.prompt, in[0].sigma, 0, 1, c->cfg.timestep_scale, m.prompt_emb, nullptr, st));
    const int fold = (m.use_comb && c->fold_norms >= 1 && m.fold_max >= 1) ? 1 : 0;
    c->text_kv_ev = nullptr;
    bool skipped = false;
    for (int l = 0; l < c->cfg.num_layers && !skipped; ++l) {
        if (l == 0) TRY(fbc_before_head(c, f, st));
        TRY(block_attention(c, 0, l, es, st, fold, false));
        TRY(block_ffn(c, 0, l, es, st));
        if (l == 0) TRY(fbc_after_head(c, f, st, skipped));
    }
    if (!skipped) TRY(fbc_after_tail(c, f, st));
    TRY(norm_mod_launch(m.x, m.D, m.h, m.D, m.N, m.D, c->cfg.norm_eps, 1, w.sst_out + m.D, w.sst_out, m.e_f, m.e_f, ee, st));
    return dense(c, gemm_dense_params(m.h, m.D, w.proj_w, w.proj_b, in[0].velocity, m.Cout, m.N, m.Cout, m.D), EPI_F32, st);
}
}  // namespace

int ltx2_dit_fbc_configure(ltx2_dit* c, int n_slots, float threshold) {
    LTX2_CHECK_ARG(c, "dit_fbc_configure: null context");
    LTX2_CHECK_ARG(n_slots >= 0 && n_slots <= 8, "dit_fbc_configure: n_slots=%d, 0 (off) to 8", n_slots);
    LTX2_CHECK_ARG(threshold >= 0.f, "dit_fbc_configure: threshold=%g must be >= 0", threshold);      // (a NaN fails it too)
    if (n_slots > 0 && c->av) {
        ltx2_set_error("dit_fbc_configure: the first-block cache is built for the VideoOnly model alone (AudioVideo contexts are not)");
        return LTX2_E_UNSUPPORTED;
    }
    LTX2_CHECK_ARG(n_slots == 0 || c->cfg.num_layers >= 2, "dit_fbc_configure: a model of one layer has no tail to reuse");
    if (FbcState* o = fbc_state(c)) {          // (hipFree waits for the passes that may still be reading the buffers)
        if ((o->fbc_buf && hipFree(o->fbc_buf) != hipSuccess) || (o->fbc_host && hipHostFree(o->fbc_host) != hipSuccess)) {
            ltx2_set_error("dit_fbc_configure: freeing the cache buffers failed");
            return LTX2_E_HIP;
        }
        fbc_states.erase(c);
    }
    if (n_slots == 0) return LTX2_OK;
    FbcState& s = fbc_states[c];
    s.D = c->m[0].D;
    s.fbc_slots.assign(n_slots, FbcSlot{});
    s.fbc_threshold = threshold;
    return LTX2_OK;
}

int ltx2_dit_fbc_reset(ltx2_dit* c) {
    LTX2_CHECK_ARG(c, "dit_fbc_reset: null context");
    FbcState* o = fbc_state(c);
    if (!o) return LTX2_OK;
    for (FbcSlot& s : o->fbc_slots) {
        s.valid = s.force = false;
        s.evals = s.skips = 0;
        s.num = s.den = 0.0;
    }
    return LTX2_OK;
}

int ltx2_dit_fbc_force_next(ltx2_dit* c, int slot) {
    FbcState* o = c ? fbc_state(c) : nullptr;
    const int n = o ? (int)o->fbc_slots.size() : 0;
    LTX2_CHECK_ARG(c && slot >= -1 && slot < n, "dit_fbc_force_next: bad context / slot (%d configured)", n);
    for (int k = 0; k < n; ++k)
        if (slot < 0 || slot == k) o->fbc_slots[k].force = true;
    return LTX2_OK;
}

int ltx2_dit_fbc_stats(const ltx2_dit* c, int slot, int64_t* evaluations, int64_t* skips, double* last_num, double* last_den) {
    const FbcState* o = c ? fbc_state(c) : nullptr;
    LTX2_CHECK_ARG(o && slot >= 0 && slot < (int)o->fbc_slots.size(), "dit_fbc_stats: bad context / slot");
    const FbcSlot& s = o->fbc_slots[slot];
    if (evaluations) *evaluations = s.evals;
    if (skips) *skips = s.skips;
    if (last_num) *last_num = s.num;
    if (last_den) *last_den = s.den;
    return LTX2_OK;
}

int ltx2_dit_forward_fbc(ltx2_dit* c, int slot, int pass_kind, const float* latent, const float* timesteps, int n_timesteps, const float* sigma,
                         float* velocity, void* stream) {
    LTX2_CHECK_ARG(c && latent && timesteps && velocity, "dit_forward_fbc: null argument");
    LTX2_CHECK_ARG(pass_kind >= LTX2_FBC_PASS_PLAIN && pass_kind <= LTX2_FBC_PASS_ISOLATED, "dit_forward_fbc: bad pass_kind %d", pass_kind);
    if (c->av || pass_kind != LTX2_FBC_PASS_PLAIN) {
        ltx2_set_error("dit_forward_fbc: the first-block cache is built for the plain pass of the VideoOnly model alone (%s is not)",
                       c->av ? "an AudioVideo model" : pass_kind == LTX2_FBC_PASS_PERTURBED ? "a perturbed (STG) pass" : "a modality-isolated pass");
        return LTX2_E_UNSUPPORTED;
    }
    TRY(check_ready(c, "dit_forward_fbc", false));
    ModIn in[1] = {{latent, timesteps, n_timesteps, sigma ? sigma : timesteps, velocity}};
    return forward_fbc(c, in, (hipStream_t)stream, {fbc_state(c), slot}, "dit_forward_fbc");
}

int ltx2_dit_denoise_step_fbc(ltx2_dit* c, int slot, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, float sigma,
                              float sigma_next, void* stream) {
    LTX2_CHECK_ARG(c && latent && timesteps, "dit_denoise_step_fbc: null argument");
    if (c->av) {
        ltx2_set_error("dit_denoise_step_fbc: the first-block cache is built for the VideoOnly model alone (AudioVideo contexts are not)");
        return LTX2_E_UNSUPPORTED;
    }
    TRY(check_ready(c, "dit_denoise_step_fbc", false));
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");
    hipStream_t st = (hipStream_t)stream;
    Mod& m = c->m[0];
    ModIn in[1] = {{latent, timesteps, n_timesteps, sigma_dev ? sigma_dev : timesteps, m.vel}};
    TRY(forward_fbc(c, in, st, {fbc_state(c), slot}, "dit_denoise_step_fbc"));
    TRY(x0_from_velocity_launch(latent, m.vel, timesteps, n_timesteps == 1 ? 0 : 1, 0.f, m.x0, m.N, m.Cout, st));
    return euler_step_launch(latent, m.x0, nullptr, nullptr, sigma, sigma_next, latent, m.N, m.Cout, st);
}

int ltx2_dit_rescaled_guided_step_fbc(ltx2_dit* c, ltx2_dit* neg, int slot_pos, int slot_neg, float* latent, const float* timesteps, int n_timesteps,
                                      const float* sigma_dev, float cfg_scale, double guidance_rescale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(c && neg && latent && timesteps, "dit_rescaled_guided_step_fbc: null argument");
    if (c->av || neg->av) {
        ltx2_set_error("dit_rescaled_guided_step_fbc: the first-block cache is built for the VideoOnly model alone (AudioVideo contexts are not)");
        return LTX2_E_UNSUPPORTED;
    }
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_rescaled_guided_step_fbc"));
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");          // before the workspace is touched
    LTX2_CHECK_ARG(slot_pos != slot_neg, "dit_rescaled_guided_step_fbc: the two passes need a slot each (both are %d)", slot_pos);
    // both passes' refusals before the first is enqueued
    const char* who = "dit_rescaled_guided_step_fbc";
    hipStream_t st = (hipStream_t)stream;
    const FbcPass pp = {fbc_state(c), slot_pos}, pn = {fbc_state(c), slot_neg};
    TRY(fbc_ready(c, pp, st, who));
    TRY(fbc_ready(neg, pn, st, who));
    const bool rescale = guidance_rescale > 0.0;
    if (rescale) TRY(rescaled_workspace(c));
    // rescaled_guided_step() with its two evaluations through the slots
    Mod& m = c->m[0];
    ModIn in[1] = {{latent, timesteps, n_timesteps, sigma_dev ? sigma_dev : timesteps, m.vel}};
    TRY(forward_fbc(c, in, st, pp, who));
    in[0].velocity = neg->m[0].vel;
    TRY(forward_fbc(neg, in, st, pn, who));
    const long stride = n_timesteps == 1 ? 0 : 1;
    if (rescale) TRY(channel_guidance_stats_launch(latent, m.vel, neg->m[0].vel, timesteps, stride, cfg_scale, c->cs_part, c->cs_stats, m.N, m.Cout, st));
    return rescaled_guided_euler_step_launch(latent, m.vel, neg->m[0].vel, timesteps, stride, rescale ? c->cs_stats : nullptr, cfg_scale, guidance_rescale,
                                             sigma, sigma_next, latent, m.N, m.Cout, st);
}

int ltx2_dit_guided_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                         const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(neg && latent && timesteps, "dit_guided_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_guided_step"));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, mask, clean);
    return guided_step(c, neg, &v.in, v.io, cfg_scale, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_rescaled_guided_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                                  float cfg_scale, double guidance_rescale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(neg && latent && timesteps, "dit_rescaled_guided_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_rescaled_guided_step"));
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");          // before the workspace is touched
    if (guidance_rescale > 0.0) TRY(rescaled_workspace(c));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, nullptr, nullptr);
    return rescaled_guided_step(c, neg, v.in, v.io, cfg_scale, guidance_rescale, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_rescaled_guided(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, float cfg_scale,
                                           double guidance_rescale, void* stream) {
    const LoopIo lo = {{latent, nullptr}, {}};
    TRY(capture_ready(c, neg, true, false, lo, host_sigmas, n_steps, "dit_graph_capture_rescaled_guided"));
    for (int i = 0; i < n_steps; ++i) LTX2_CHECK_ARG(host_sigmas[i] != 0.f, "Sigma can't be 0.0");
    if (guidance_rescale > 0.0) TRY(rescaled_workspace(c));
    LoopStep step;
    step.neg = neg;
    step.cfg_scale = cfg_scale;
    step.rescaled = true;
    step.guidance_rescale = guidance_rescale;
    return capture_loop(c, step, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_guided_step_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, const float* a_latent, const float* v_timesteps, int n_v_timesteps,
                            const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                            float cfg_scale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(neg && v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_guided_step_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_guided_step_av"));
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    // the audio latent is read by both evaluations and never written
    const ModIn in[2] = {v.in, step_args(const_cast<float*>(a_latent), a_timesteps, n_a_timesteps, sigma_dev, nullptr, nullptr).in};
    return guided_step(c, neg, in, v.io, cfg_scale, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_guided_step_joint_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                                  const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                                  const float* a_mask, const float* a_clean, float cfg_scale, float audio_cfg_scale, float sigma, float sigma_next,
                                  void* stream) {
    LTX2_CHECK_ARG(neg && v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_guided_step_joint_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_guided_step_joint_av"));
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    const StepArgs a = step_args(a_latent, a_timesteps, n_a_timesteps, sigma_dev, a_mask, a_clean);
    const ModIn in[2] = {v.in, a.in};
    const StepIo io[2] = {v.io, a.io};
    const float cfg[2] = {cfg_scale, audio_cfg_scale};
    return guided_step_joint(c, neg, in, io, cfg, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_ancestral_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, const float* mask,
                            const float* clean, float cfg_scale, float sigma, float sigma_up, float sigma_down, const uint64_t* seed_dev, uint32_t step,
                            void* stream) {
    LTX2_CHECK_ARG(latent && timesteps, "dit_ancestral_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_ancestral_step"));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, mask, clean);
    const float cfg[2] = {cfg_scale, 0.f};
    return ancestral_step(c, neg, &v.in, &v.io, cfg, sigma, {sigma_up, sigma_down, seed_dev, step}, (hipStream_t)stream);
}

int ltx2_dit_ancestral_step_joint_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                                     const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                                     const float* a_mask, const float* a_clean, float cfg_scale, float audio_cfg_scale, float sigma, float sigma_up,
                                     float sigma_down, const uint64_t* seed_dev, uint32_t step, void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_ancestral_step_joint_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_ancestral_step_joint_av"));
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    const StepArgs a = step_args(a_latent, a_timesteps, n_a_timesteps, sigma_dev, a_mask, a_clean);
    const ModIn in[2] = {v.in, a.in};
    const StepIo io[2] = {v.io, a.io};
    const float cfg[2] = {cfg_scale, audio_cfg_scale};
    return ancestral_step(c, neg, in, io, cfg, sigma, {sigma_up, sigma_down, seed_dev, step}, (hipStream_t)stream);
}

namespace {
// what both ancestral capture entries check of their per-step scalars and their seed, before the capture begins
int ancestral_capture_check(const float* up, const float* down, int n_steps, const uint64_t* seed_dev, const char* who) {
    LTX2_CHECK_ARG(up && down, "%s: bad argument", who);
    for (int i = 0; i < n_steps; ++i) LTX2_CHECK_ARG(up[i] >= 0.f && down[i] >= 0.f, "%s: sigma_up=%g and sigma_down=%g must be >= 0", who, up[i], down[i]);
    LTX2_CHECK_ARG(seed_dev && ((uintptr_t)seed_dev & 7) == 0, "%s: seed_dev is a device pointer to one 8-byte aligned 64-bit word", who);
    return LTX2_OK;
}
}  // namespace

int ltx2_dit_graph_capture_ancestral(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask,
                                     const float* clean, int64_t n_clean, float cfg_scale, const float* host_sigma_up, const float* host_sigma_down,
                                     const uint64_t* seed_dev, void* stream) {
    const LoopIo lo = {{latent, nullptr}, {{mask, (long)n_mask, clean, (long)n_clean}, {}}};
    TRY(capture_ready(c, neg, false, false, lo, host_sigmas, n_steps, "dit_graph_capture_ancestral"));
    TRY(ancestral_capture_check(host_sigma_up, host_sigma_down, n_steps, seed_dev, "dit_graph_capture_ancestral"));
    LoopStep step;
    step.neg = neg;
    step.cfg_scale = cfg_scale;
    step.ancestral_up = host_sigma_up;
    step.ancestral_down = host_sigma_down;
    step.ancestral_seed = seed_dev;
    return capture_loop(c, step, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_ancestral_joint_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                                              const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask,
                                              int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, float cfg_scale, float audio_cfg_scale,
                                              const float* host_sigma_up, const float* host_sigma_down, const uint64_t* seed_dev,
                                              void* stream) {
    const LoopIo lo = {{v_latent, a_latent}, {{v_mask, (long)n_v_mask, v_clean, (long)n_v_clean}, {a_mask, (long)n_a_mask, a_clean, (long)n_a_clean}}};
    TRY(capture_ready(c, neg, false, true, lo, host_sigmas, n_steps, "dit_graph_capture_ancestral_joint_av", true));
    TRY(ancestral_capture_check(host_sigma_up, host_sigma_down, n_steps, seed_dev, "dit_graph_capture_ancestral_joint_av"));
    LoopStep step;
    step.neg = neg;
    step.cfg_scale = cfg_scale;
    step.joint = true;
    step.audio_cfg_scale = audio_cfg_scale;
    step.ancestral_up = host_sigma_up;
    step.ancestral_down = host_sigma_down;
    step.ancestral_seed = seed_dev;
    return capture_loop(c, step, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_stg_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, const float* mask,
                      const float* clean, float* vel_perturbed, float cfg_scale, float stg_scale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(latent && timesteps, "dit_stg_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_stg_step"));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, mask, clean);
    return stg_step(c, neg, v.in, v.io, vel_perturbed, cfg_scale, stg_scale, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_stg_step_joint_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                               const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                               const float* a_mask, const float* a_clean, float* v_vel_perturbed, int64_t n_v_vel, float* a_vel_perturbed, int64_t n_a_vel,
                               float cfg_scale, float audio_cfg_scale, float stg_scale, float audio_stg_scale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_stg_step_joint_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_stg_step_joint_av"));
    float* const ptb[2] = {v_vel_perturbed, a_vel_perturbed};
    const int64_t n_ptb[2] = {n_v_vel, n_a_vel};
    const float cfg[2] = {cfg_scale, audio_cfg_scale}, stg[2] = {stg_scale, audio_stg_scale};
    LTX2_CHECK_ARG(ptb[0] && ptb[1], "dit_stg_step_joint_av: v_vel_perturbed and a_vel_perturbed (fp32 scratch, [N][out_channels] and [Na][audio_out_channels]) "
                                     "are both required: the perturbed pass writes both modalities' velocities");
    LTX2_CHECK_ARG(stg[0] != 0.f || stg[1] != 0.f, "dit_stg_step_joint_av: both STG scales are 0: that is ltx2_dit_guided_step_joint_av (ltx2_dit_denoise_step_av "
                                                   "without a negative context)");
    for (int k = 0; k < 2; ++k) {
        // the perturbed pass writes, and the step kernel reads, N * out_channels elements of each scratch: another length would be an out-of-bounds
        // access, not an error (the comment at cond_modality())
        const int64_t need = (int64_t)c->m[k].N * c->m[k].Cout;
        LTX2_CHECK_ARG(n_ptb[k] == need, "dit_stg_step_joint_av: modality %d has %d tokens x %d channels, got a perturbed scratch of %ld elements", k, c->m[k].N,
                       c->m[k].Cout, (long)n_ptb[k]);
        bool any = false;
        for (unsigned char f : c->stg[k]) any = any || f != 0;
        LTX2_CHECK_ARG(stg[k] == 0.f || any, "dit_stg_step_joint_av: the %s STG scale is %g but no %s self-attention is marked (ltx2_dit_set_stg_blocks, modality %d)",
                       k ? "audio" : "video", (double)stg[k], k ? "audio" : "video", k);
    }
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    const StepArgs a = step_args(a_latent, a_timesteps, n_a_timesteps, sigma_dev, a_mask, a_clean);
    const ModIn in[2] = {v.in, a.in};
    const StepIo io[2] = {v.io, a.io};
    return stg_step_joint(c, neg, in, io, ptb, cfg, stg, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_projected_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, const float* mask,
                            const float* clean, int mode, float scale, float eta, float norm_threshold, float momentum, int first, float sigma,
                            float sigma_next, void* stream) {
    LTX2_CHECK_ARG(neg && latent && timesteps, "dit_projected_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_projected_step"));
    const Projected g = {mode, scale, eta, norm_threshold, momentum};
    TRY(projected_check(g, "dit_projected_step"));
    TRY(projected_workspace(c, g.running(), first == 0));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, mask, clean);
    return projected_step(c, neg, v.in, v.io, g, first, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_projected_step_joint_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                                     const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                                     const float* a_mask, const float* a_clean, int v_mode, float v_scale, float v_eta, float v_norm_threshold,
                                     float v_momentum, float* v_running, int64_t n_v_running, int a_mode, float a_scale, float a_eta,
                                     float a_norm_threshold, float a_momentum, float* a_running, int64_t n_a_running, int first, float sigma,
                                     float sigma_next, void* stream) {
    LTX2_CHECK_ARG(neg && v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_projected_step_joint_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_projected_step_joint_av"));
    const Projected g[2] = {{v_mode, v_scale, v_eta, v_norm_threshold, v_momentum}, {a_mode, a_scale, a_eta, a_norm_threshold, a_momentum}};
    float* const run[2] = {v_running, a_running};
    const int64_t n_run[2] = {n_v_running, n_a_running};
    TRY(projected_joint_check(g, run, n_run, c, "dit_projected_step_joint_av"));
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    const StepArgs a = step_args(a_latent, a_timesteps, n_a_timesteps, sigma_dev, a_mask, a_clean);
    const ModIn in[2] = {v.in, a.in};
    const StepIo io[2] = {v.io, a.io};
    TRY(step_check(sigma, io, 2, "dit_projected_step_joint_av"));        // every refusal stands before the workspace is touched
    TRY(projected_joint_workspace(c, g));
    return projected_step_joint(c, neg, in, io, g, run, first, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_res2s_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                        const float* ts_sub, const float* sub_sigma_dev, const float* mask, const float* clean, float cfg_scale, float sigma,
                        float sigma_next, void* stream) {
    LTX2_CHECK_ARG(latent && timesteps, "dit_res2s_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_res2s_step"));
    Res2sPlan p;
    TRY(res2s_plan(sigma, sigma_next, p));
    LTX2_CHECK_ARG(p.last || ts_sub, "dit_res2s_step: ts_sub is needed unless the step is the final one");
    TRY(res2s_workspace(c, res2s_total(c)));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, mask, clean);
    return res2s_step(c, neg, &v.in, ts_sub, nullptr, sub_sigma_dev ? sub_sigma_dev : ts_sub, nullptr, &v.io, cfg_scale, 0.f, p, (hipStream_t)stream);
}

int ltx2_dit_res2s_step_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                           const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_ts_sub, const float* a_ts_sub,
                           const float* sub_sigma_dev, const float* v_mask, const float* v_clean, const float* a_mask, const float* a_clean,
                           float cfg_scale, float audio_cfg_scale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_res2s_step_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_res2s_step_av"));
    Res2sPlan p;
    TRY(res2s_plan(sigma, sigma_next, p));
    LTX2_CHECK_ARG(p.last || (v_ts_sub && a_ts_sub), "dit_res2s_step_av: v_ts_sub and a_ts_sub are needed unless the step is the final one");
    TRY(res2s_workspace(c, res2s_total(c)));
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    const StepArgs a = step_args(a_latent, a_timesteps, n_a_timesteps, sigma_dev, a_mask, a_clean);
    const ModIn in[2] = {v.in, a.in};
    const StepIo io[2] = {v.io, a.io};
    return res2s_step(c, neg, in, v_ts_sub, a_ts_sub, sub_sigma_dev ? sub_sigma_dev : v_ts_sub, nullptr, io, cfg_scale, audio_cfg_scale, p, (hipStream_t)stream);
}

int ltx2_dit_heun_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, const float* ts_next,
                       const float* sigma_next_dev, const float* mask, const float* clean, float cfg_scale, float ge_gamma, int first, float sigma,
                       float sigma_next, void* stream) {
    LTX2_CHECK_ARG(latent && timesteps, "dit_heun_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_heun_step"));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, mask, clean);
    TRY(heun_check(c, &v.io, ge_gamma, sigma, sigma_next, "dit_heun_step"));
    LTX2_CHECK_ARG(sigma_next == 0.f || ts_next, "dit_heun_step: ts_next is needed unless sigma_next is 0");
    TRY(heun_workspace(c, ge_gamma > 0.f && first == 0));
    const float* const next[2] = {ts_next, nullptr};
    const float cfg[2] = {cfg_scale, 0.f};
    TRY(heun_step(c, neg, &v.in, next, sigma_next_dev ? sigma_next_dev : ts_next, nullptr, &v.io, cfg, ge_gamma, first, sigma, sigma_next, (hipStream_t)stream));
    c->heun_prev = c->heun_prev || (ge_gamma > 0.f && first != 0);
    return LTX2_OK;
}

int ltx2_dit_heun_step_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                          const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_ts_next, const float* a_ts_next,
                          const float* sigma_next_dev, const float* v_mask, const float* v_clean, const float* a_mask, const float* a_clean,
                          float cfg_scale, float audio_cfg_scale, float ge_gamma, int first, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_heun_step_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_heun_step_av"));
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    const StepArgs a = step_args(a_latent, a_timesteps, n_a_timesteps, sigma_dev, a_mask, a_clean);
    const ModIn in[2] = {v.in, a.in};
    const StepIo io[2] = {v.io, a.io};
    TRY(heun_check(c, io, ge_gamma, sigma, sigma_next, "dit_heun_step_av"));
    LTX2_CHECK_ARG(sigma_next == 0.f || (v_ts_next && a_ts_next), "dit_heun_step_av: v_ts_next and a_ts_next are needed unless sigma_next is 0");
    TRY(heun_workspace(c, ge_gamma > 0.f && first == 0));
    const float* const next[2] = {v_ts_next, a_ts_next};
    const float cfg[2] = {cfg_scale, audio_cfg_scale};
    TRY(heun_step(c, neg, in, next, sigma_next_dev ? sigma_next_dev : v_ts_next, nullptr, io, cfg, ge_gamma, first, sigma, sigma_next, (hipStream_t)stream));
    c->heun_prev = c->heun_prev || (ge_gamma > 0.f && first != 0);
    return LTX2_OK;
}

int ltx2_dit_ge_step(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, const float* mask,
                     const float* clean, float cfg_scale, float ge_gamma, int first, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(latent && timesteps, "dit_ge_step: null argument");
    const int n_ts[2] = {n_timesteps, 1};
    TRY(step_ready(c, neg, false, n_ts, "dit_ge_step"));
    const StepArgs v = step_args(latent, timesteps, n_timesteps, sigma_dev, mask, clean);
    TRY(heun_check(c, &v.io, ge_gamma, sigma, sigma_next, "dit_ge_step"));
    LTX2_CHECK_ARG(ge_gamma > 0.f, "dit_ge_step: ge_gamma=%g must be > 0 (without GE the step is ltx2_dit_guided_step or ltx2_dit_denoise_step)", ge_gamma);
    TRY(heun_workspace(c, first == 0));
    TRY(ge_step(c, neg, v.in, v.io, cfg_scale, ge_gamma, first, sigma, sigma_next, (hipStream_t)stream));
    c->heun_prev = c->heun_prev || first != 0;
    return LTX2_OK;
}

int ltx2_dit_graph_capture_heun(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask,
                                const float* clean, int64_t n_clean, float cfg_scale, float ge_gamma, void* stream) {
    const LoopIo lo = {{latent, nullptr}, {{mask, (long)n_mask, clean, (long)n_clean}, {}}};
    TRY(capture_ready(c, neg, false, false, lo, host_sigmas, n_steps, "dit_graph_capture_heun"));
    LTX2_CHECK_ARG(ge_gamma >= 0.f, "dit_graph_capture_heun: ge_gamma=%g must be >= 0 (0: no GE)", ge_gamma);
    for (int i = 0; i < n_steps; ++i)
        LTX2_CHECK_ARG(host_sigmas[i] > 0.f && host_sigmas[i + 1] >= 0.f, "dit_graph_capture_heun: sigma=%g must be > 0 and sigma_next=%g >= 0", host_sigmas[i],
                       host_sigmas[i + 1]);
    TRY(heun_workspace(c, false));
    LoopStep step;
    step.neg = neg;
    step.cfg_scale = cfg_scale;
    step.heun = true;
    step.ge_gamma = ge_gamma;
    return capture_loop(c, step, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_mm_guided_step_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                               const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                               const float* a_mask, const float* a_clean, float* v_vel_isolated, int64_t n_v_isolated, float* a_vel_isolated,
                               int64_t n_a_isolated, float* v_vel_perturbed, int64_t n_v_perturbed, float* a_vel_perturbed, int64_t n_a_perturbed,
                               float v_cfg_scale, float v_stg_scale, float v_modality_scale, float v_rescale_scale, float a_cfg_scale, float a_stg_scale,
                               float a_modality_scale, float a_rescale_scale, float sigma, float sigma_next, void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && v_timesteps && a_timesteps && sigma_dev, "dit_mm_guided_step_av: null argument");
    const int n_ts[2] = {n_v_timesteps, n_a_timesteps};
    TRY(step_ready(c, neg, true, n_ts, "dit_mm_guided_step_av"));
    float* const mod[2] = {v_vel_isolated, a_vel_isolated};
    float* const ptb[2] = {v_vel_perturbed, a_vel_perturbed};
    const int64_t n_mod[2] = {n_v_isolated, n_a_isolated}, n_ptb[2] = {n_v_perturbed, n_a_perturbed};
    // the passes write, and the step kernels read, N * out_channels elements of each scratch: another length would be an out-of-bounds access, not an
    // error (the comment at cond_modality())
    for (int k = 0; k < 2; ++k) {
        const int64_t need = (int64_t)c->m[k].N * c->m[k].Cout;
        LTX2_CHECK_ARG((!mod[k] || n_mod[k] == need) && (!ptb[k] || n_ptb[k] == need),
                       "dit_mm_guided_step_av: modality %d has %d tokens x %d channels, got an isolated scratch of %ld and a perturbed scratch of %ld elements", k,
                       c->m[k].N, c->m[k].Cout, (long)(mod[k] ? n_mod[k] : need), (long)(ptb[k] ? n_ptb[k] : need));
    }
    const MmGuide g[2] = {{v_cfg_scale, v_stg_scale, v_modality_scale, v_rescale_scale}, {a_cfg_scale, a_stg_scale, a_modality_scale, a_rescale_scale}};
    const StepArgs v = step_args(v_latent, v_timesteps, n_v_timesteps, sigma_dev, v_mask, v_clean);
    const StepArgs a = step_args(a_latent, a_timesteps, n_a_timesteps, sigma_dev, a_mask, a_clean);
    const ModIn in[2] = {v.in, a.in};
    const StepIo io[2] = {v.io, a.io};
    // every refusal of the step itself stands before the workspace is touched and before anything is enqueued
    TRY(step_check(sigma, io, 2, "dit_mm_guided_step_av"));
    LTX2_CHECK_ARG((mod[0] == nullptr) == (mod[1] == nullptr) && (ptb[0] == nullptr) == (ptb[1] == nullptr),
                   "dit_mm_guided_step_av: a pass writes both modalities' velocities: its video and audio scratch go together");
    LTX2_CHECK_ARG(!ptb[0] || !c->stg[0].empty() || !c->stg[1].empty(),
                   "dit_mm_guided_step_av: a perturbed scratch is given but no self-attention is marked (ltx2_dit_set_stg_blocks)");
    TRY(mm_workspace(c, g));
    return mm_guided_step(c, neg, in, io, mod, ptb, g, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_dit_graph_capture(ltx2_dit* c, float* latent, const float* host_sigmas, int n_steps, void* stream) {
    LTX2_CHECK_ARG(latent && host_sigmas && n_steps > 0 && n_steps < 64, "dit_graph_capture: bad argument");
    TRY(check_ready(c, "dit_graph_capture", false));
    float* const lat[2] = {latent, nullptr};
    const Cond none[2] = {};
    return capture_loop(c, {}, lat, none, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_cond(ltx2_dit* c, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask, const float* clean,
                                int64_t n_clean, void* stream) {
    LTX2_CHECK_ARG(latent && host_sigmas && n_steps > 0 && n_steps < 64, "dit_graph_capture_cond: bad argument");
    TRY(check_ready(c, "dit_graph_capture_cond", false));
    float* const lat[2] = {latent, nullptr};
    const Cond cond[2] = {{mask, (long)n_mask, clean, (long)n_clean}, {}};
    return capture_loop(c, {}, lat, cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_guided(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask,
                                  int64_t n_mask, const float* clean, int64_t n_clean, float cfg_scale, void* stream) {
    const LoopIo lo = {{latent, nullptr}, {{mask, (long)n_mask, clean, (long)n_clean}, {}}};
    TRY(capture_ready(c, neg, true, false, lo, host_sigmas, n_steps, "dit_graph_capture_guided"));
    return capture_loop(c, {neg, cfg_scale}, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_stg(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask,
                               const float* clean, int64_t n_clean, float* vel_perturbed, int64_t n_vel, float cfg_scale, float stg_scale, double stg_cutoff,
                               void* stream) {
    LTX2_CHECK_ARG(vel_perturbed, "dit_graph_capture_stg: bad argument");
    const LoopIo lo = {{latent, nullptr}, {{mask, (long)n_mask, clean, (long)n_clean}, {}}};
    TRY(capture_ready(c, neg, false, false, lo, host_sigmas, n_steps, "dit_graph_capture_stg"));
    // every replayed STG step writes N * out_channels velocities there
    LTX2_CHECK_ARG(n_vel == (int64_t)c->m[0].N * c->m[0].Cout, "dit_graph_capture_stg: vel_perturbed has %ld elements, %d tokens x %d channels are needed", (long)n_vel,
                   c->m[0].N, c->m[0].Cout);
    // step i is an STG step iff (i + 1) / n_steps <= stg_cutoff (one_stage.py:289-294), in double as Python divides; the fractions grow with i
    int stg_steps = 0;
    while (stg_steps < n_steps && (double)(stg_steps + 1) / (double)n_steps <= stg_cutoff) ++stg_steps;
    LoopStep step;
    step.neg = neg;
    step.cfg_scale = cfg_scale;
    step.stg_vel = vel_perturbed;
    step.stg_scale = stg_scale;
    step.stg_steps = stg_steps;
    return capture_loop(c, step, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_projected(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask,
                                     const float* clean, int64_t n_clean, int mode, float scale, float eta, float norm_threshold, float momentum,
                                     void* stream) {
    const LoopIo lo = {{latent, nullptr}, {{mask, (long)n_mask, clean, (long)n_clean}, {}}};
    TRY(capture_ready(c, neg, true, false, lo, host_sigmas, n_steps, "dit_graph_capture_projected"));
    const Projected g = {mode, scale, eta, norm_threshold, momentum};
    TRY(projected_check(g, "dit_graph_capture_projected"));
    TRY(projected_workspace(c, g.running(), false));
    return capture_loop(c, {neg, 0.f, &g}, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_res2s(ltx2_dit* c, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask,
                                 int64_t n_mask, const float* clean, int64_t n_clean, float cfg_scale, void* stream) {
    const LoopIo lo = {{latent, nullptr}, {{mask, (long)n_mask, clean, (long)n_clean}, {}}};
    TRY(capture_ready(c, neg, false, false, lo, host_sigmas, n_steps, "dit_graph_capture_res2s"));
    Res2sPlan plan[64];
    for (int i = 0; i < n_steps; ++i) TRY(res2s_plan(host_sigmas[i], host_sigmas[i + 1], plan[i]));
    TRY(res2s_workspace(c, res2s_total(c)));
    return capture_loop(c, {neg, cfg_scale, nullptr, plan}, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_cond_av(ltx2_dit* c, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps, const float* v_mask, int64_t n_v_mask,
                                   const float* v_clean, int64_t n_v_clean, const float* a_mask, int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && host_sigmas && n_steps > 0 && n_steps < 64, "dit_graph_capture_cond_av: bad argument");
    TRY(check_ready(c, "dit_graph_capture_cond_av", true));
    float* const lat[2] = {v_latent, a_latent};
    const Cond cond[2] = {{v_mask, (long)n_v_mask, v_clean, (long)n_v_clean}, {a_mask, (long)n_a_mask, a_clean, (long)n_a_clean}};
    return capture_loop(c, {}, lat, cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_guided_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, const float* a_latent, const float* host_sigmas, int n_steps,
                                     const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask, int64_t n_a_mask,
                                     float cfg_scale, void* stream) {
    // the audio latent is read by both evaluations and never written: its mask gives the timesteps only
    const LoopIo lo = {{v_latent, const_cast<float*>(a_latent)}, {{v_mask, (long)n_v_mask, v_clean, (long)n_v_clean}, {a_mask, (long)n_a_mask, nullptr, 0}}};
    TRY(capture_ready(c, neg, true, true, lo, host_sigmas, n_steps, "dit_graph_capture_guided_av"));
    return capture_loop(c, {neg, cfg_scale}, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_guided_joint_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                                           const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask,
                                           int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, float cfg_scale, float audio_cfg_scale, void* stream) {
    const LoopIo lo = {{v_latent, a_latent}, {{v_mask, (long)n_v_mask, v_clean, (long)n_v_clean}, {a_mask, (long)n_a_mask, a_clean, (long)n_a_clean}}};
    TRY(capture_ready(c, neg, true, true, lo, host_sigmas, n_steps, "dit_graph_capture_guided_joint_av", true));
    LoopStep step;
    step.neg = neg;
    step.cfg_scale = cfg_scale;
    step.joint = true;
    step.audio_cfg_scale = audio_cfg_scale;
    return capture_loop(c, step, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_projected_joint_av(ltx2_dit* c, ltx2_dit* neg, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                                              const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask,
                                              int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, int v_mode, float v_scale, float v_eta,
                                              float v_norm_threshold, float v_momentum, float* v_running, int64_t n_v_running, int a_mode,
                                              float a_scale, float a_eta, float a_norm_threshold, float a_momentum, float* a_running,
                                              int64_t n_a_running, void* stream) {
    const LoopIo lo = {{v_latent, a_latent}, {{v_mask, (long)n_v_mask, v_clean, (long)n_v_clean}, {a_mask, (long)n_a_mask, a_clean, (long)n_a_clean}}};
    TRY(capture_ready(c, neg, true, true, lo, host_sigmas, n_steps, "dit_graph_capture_projected_joint_av", true));
    const Projected g[2] = {{v_mode, v_scale, v_eta, v_norm_threshold, v_momentum}, {a_mode, a_scale, a_eta, a_norm_threshold, a_momentum}};
    float* const run[2] = {v_running, a_running};
    const int64_t n_run[2] = {n_v_running, n_a_running};
    TRY(projected_joint_check(g, run, n_run, c, "dit_graph_capture_projected_joint_av"));
    TRY(projected_joint_workspace(c, g));
    LoopStep step;
    step.neg = neg;
    step.joint = true;
    step.projected_joint = g;
    step.running_joint = run;
    return capture_loop(c, step, lo.lat, lo.cond, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_graph_capture_av(ltx2_dit* c, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                              void* stream) {
    LTX2_CHECK_ARG(v_latent && a_latent && host_sigmas && n_steps > 0 && n_steps < 64, "dit_graph_capture_av: bad argument");
    TRY(check_ready(c, "dit_graph_capture_av", true));
    float* const lat[2] = {v_latent, a_latent};
    const Cond none[2] = {};
    return capture_loop(c, {}, lat, none, host_sigmas, n_steps, (hipStream_t)stream);
}

int ltx2_dit_profile_begin(ltx2_dit* c, int epilogue) {
    LTX2_CHECK_ARG(c && epilogue >= -1 && epilogue < EPI_COUNT, "dit_profile_begin: bad argument");
    c->prof_epi = epilogue;
    c->prof_used = 0;
    c->prof_flops = 0;
    g_prof_ctx = c;
    return LTX2_OK;
}

int ltx2_dit_profile_end(ltx2_dit* c, double* total_ms, int64_t* launches, double* flops) {
    LTX2_CHECK_ARG(c && total_ms && launches && flops, "dit_profile_end: null argument");
    g_prof_ctx = nullptr;
    c->prof_epi = -2;
    double tot = 0;
    for (size_t i = 0; i + 1 < c->prof_used; i += 2) {
        if (hipEventSynchronize(c->prof_ev[i + 1]) != hipSuccess) {
            ltx2_set_error("dit_profile_end: event synchronize failed");
            return LTX2_E_HIP;
        }
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]);
        tot += ms;
    }
    *total_ms = tot;
    *launches = (int64_t)(c->prof_used / 2);
    *flops = c->prof_flops;
    return LTX2_OK;
}

int ltx2_dit_set_context_mask(ltx2_dit* c, int modality, const float* mask, int S, void* stream) {
    LTX2_CHECK_ARG(c && (modality == 0 || (modality == 1 && c->av)), "dit_set_context_mask: bad context / modality");
    Mod& m = c->m[modality];
    if (!c->ws) {
        ltx2_set_error("dit_set_context_mask: no workspace bound");
        return LTX2_E_STATE;
    }
    if (!mask) {
        m.has_kmask = false;
        return LTX2_OK;
    }
    LTX2_CHECK_ARG(S == m.S, "dit_set_context_mask: S=%d differs from the bound workspace S=%d", S, m.S);
    TRY(keymask_words_launch(mask, S, m.kmask, m.Spad / 64, (hipStream_t)stream));
    m.has_kmask = true;
    return LTX2_OK;
}

int ltx2_dit_set_option(ltx2_dit* c, const char* name, int value) {
    LTX2_CHECK_ARG(c && name, "dit_set_option: null argument");
    if (!strcmp(name, "fp8_compute")) {
        if (c->ws && (value != 0) != c->fp8_compute) {
            ltx2_set_error("dit_set_option: fp8_compute must be set before the workspace is bound");
            return LTX2_E_STATE;
        }
        c->fp8_compute = value != 0;
        return LTX2_OK;
    }
    if (!strcmp(name, "text_kv_ahead")) {       // 0: the video stream projects its sigma-modulated text K / V inline (round 4's schedule; same results bit for bit)
        c->text_kv_ahead = value != 0;
        return LTX2_OK;
    }
    if (!strcmp(name, "fold_norms")) {          // 0 / 1: see block_attention(); 0 restores round 5's norm pass in front of the text cross-attention
        LTX2_CHECK_ARG(value == 0 || value == 1, "dit_set_option: fold_norms is 0 or 1");
        c->fold_norms = value;
        return LTX2_OK;
    }
    if (!strcmp(name, "adaln_combine")) {       // 0: tables and embeddings reach every kernel separately (round 3's form; same results bit for bit)
        c->adaln_combine = value != 0;
        return LTX2_OK;
    }
    ltx2_set_error("dit_set_option: unknown option '%s'", name);
    return LTX2_E_INVALID;
}


int ltx2_dit_graph_launch(ltx2_dit* c, void* stream) {
    LTX2_CHECK_ARG(c, "dit_graph_launch: null context");
    if (!c->exec) {
        ltx2_set_error("dit_graph_launch: no captured graph");
        return LTX2_E_STATE;
    }
    if (hipGraphLaunch(c->exec, (hipStream_t)stream) != hipSuccess) {
        ltx2_set_error("dit_graph_launch: hipGraphLaunch failed");
        return LTX2_E_HIP;
    }
    return LTX2_OK;
}

}  // extern "C"
