// C ABI of the SigLIP text tower: `model.encode_text(tokens)` of clip_server.py:98 followed by the
// normalisation (:99) and fp16 serialisation (:166).  The reference holds no restatement of this tower (it is
// open_clip's TextTransformer, third-party and absent): known from the repository are the output width
// (model.text.text_projection.out_features, clip_server.py:107,182) and the constants of
// misc/clip_accursed.py:31-55 (width 1152, 27 layers, context 64, vocabulary 32000, pad id 1).  Published
// architecture: token + positional embedding, pre-LN blocks WITHOUT causal mask, final LayerNorm, the last
// position pooled, Linear projection with bias.  Weight names follow open_clip (`text.*`).  The blocks run on
// the same kernels as the image tower (siglip_kernels.hip).  Tokenisation stays on the host (Python).
#include "../../include/mse.h"
#include "runtime.h"
#include "siglip_encoder.h"
#include <new>
#include <string>
#include <vector>

using namespace mse;
using namespace mse::siglip;

namespace {
// rows of a part (a range of sequences on one stream) from which the LayerNorm-fused batch kernels are used: below, launch_gemm picks
// the small-batch tiles (<= 3072 rows), which have no fused form
constexpr int FUSED_MIN_ROWS = 3072;
}  // namespace

// Geometry, weight store, blocks and their activations: Encoder (siglip_encoder.h); here what only the text tower has
struct mse_siglip_text : Encoder {
    mse_siglip_text_config cfg{};
    int ctx = 0;
    static constexpr int MAX_PARTS = 4;
    hipStream_t part_s[MAX_PARTS] = {};                // streams of the parts of a large batch beyond the first (index 0 unused)
    hipEvent_t ev_fork = nullptr, part_join[MAX_PARTS] = {};
    int n_parts = 2;                                   // parts a batch of >= 32 texts runs as (MSE_SIGLIP_TEXT_PARTS)
    hipStream_t side[MAX_PARTS] = {};                  // per part: where the 128-column remainder launches of its GEMMs run
    hipEvent_t side_ev[MAX_PARTS][2] = {};
    std::mutex call_mu;   // one call at a time: token upload, kernels and scratch of a call share one stream (see mse_siglip)
    float *tok_emb = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *bproj = nullptr;
    uint16_t* wproj = nullptr;
    int64_t* tokens_dev = nullptr;
    float *pooled = nullptr, *feat = nullptr, *out_f32 = nullptr;
    uint16_t* out_f16 = nullptr;
};

extern "C" {

mse_siglip_text* mse_siglip_text_create(const mse_siglip_text_config* c) {
    if (!c) { fail("null config"); return nullptr; }
    if (c->width % 128 || c->heads <= 0 || c->width / c->heads != 72 || c->context_length % 32 || c->context_length <= 0 ||
        c->vocab_size <= 0 || c->max_batch <= 0) {
        fail("siglip text: unsupported geometry (width % 128 == 0, head_dim == 72, context % 32 == 0 required)");
        return nullptr;
    }
    mse_siglip_text* m = new (std::nothrow) mse_siglip_text();
    if (!m) { fail("out of host memory"); return nullptr; }
    m->cfg = *c;
    m->what = "siglip text"; m->eps = c->eps; m->gelu_tanh = c->gelu_tanh;
    m->D = c->width; m->H = c->heads; m->dh = m->D / m->H; m->mlp = c->mlp_dim; m->mlp_pad = (int)round_up(m->mlp, 128);
    m->ctx = c->context_length; m->n_pad = m->ctx; m->max_batch = c->max_batch;
    m->m_pad = round_up((size_t)m->max_batch * m->ctx, 256);
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { delete m; fail("hipStreamCreate failed"); return nullptr; }
    {
        const char* e = getenv("MSE_SIGLIP_TEXT_PARTS");
        m->n_parts = std::min(std::max(e ? atoi(e) : 2, 1), (int)mse_siglip_text::MAX_PARTS);
    }
    if (hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); m->n_parts = 1; }
    for (int pt = 1; pt < m->n_parts; pt++)
        if (hipStreamCreateWithFlags(&m->part_s[pt], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&m->part_join[pt], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            m->n_parts = pt;   // fewer streams then: correct, only slower
            break;
        }
    for (int hlf = 0; hlf < m->n_parts; hlf++)
        if (hipStreamCreateWithFlags(&m->side[hlf], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&m->side_ev[hlf][0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&m->side_ev[hlf][1], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (m->side[hlf]) { (void)hipStreamDestroy(m->side[hlf]); m->side[hlf] = nullptr; }
        }
    const size_t D = m->D, MP = m->mlp_pad, DP = round_up(m->D, 256);
    m->dp = (int)DP;
    m->add_f32("text.token_embedding.weight", &m->tok_emb, c->vocab_size, D);
    m->add_f32("text.positional_embedding", &m->pos, m->ctx, D);
    m->add_blocks(c->layers, BlockNames{"text.transformer.resblocks.", "ln_1.weight", "ln_1.bias", "attn.in_proj_weight",
                                        "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_2.weight", "ln_2.bias",
                                        "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"});
    {
        const char* e = getenv("MSE_SIGLIP_NOFUSE");
        m->fused = !(e && atoi(e)) && gemm_fused_ok((int)m->m_pad, (int)D, (int)MP, m->H, m->dh, m->ctx, m->n_pad, 8) &&
                   m->m_pad > (size_t)FUSED_MIN_ROWS;
    }
    const bool fused_alloc_ok = !m->fused || m->alloc_fused();
    m->add_f32("text.ln_final.weight", &m->lnf_g, 1, D); m->add_f32("text.ln_final.bias", &m->lnf_b, 1, D);
    m->add_bf16("text.text_projection.weight", &m->wproj, D, D, D, D); m->add_f32("text.text_projection.bias", &m->bproj, 1, D);
    const size_t B = m->max_batch, M = m->m_pad, BH = B * m->H;
    m->tokens_dev = m->dalloc<int64_t>(B * m->ctx);
    m->x = m->dalloc<uint16_t>(M * D, true);
    m->h = m->dalloc<uint16_t>(M * D, true);
    m->dlt = m->dalloc<uint16_t>(M * D, true);
    m->kparts = m->dalloc<float>((size_t)4 * 768 * D, true);   // K-split partial sums of fc2 for up to 12 texts (4 ranges x 768 rows)
    m->mlp_h = m->dalloc<uint16_t>(M * MP, true);
    // + 4 sequences of slack: the GEMM epilogues store the rows of the M padding (up to 255) unconditionally
    m->qb = m->dalloc<uint16_t>((BH + 4 * m->H) * m->n_pad * m->dh_pad, true);
    m->kb = m->dalloc<uint16_t>((BH + 4 * m->H) * m->n_pad * attention_k_stride(), true);
    m->vtb = m->dalloc<uint16_t>((BH + 4 * m->H) * m->dv_pad * m->n_pad, true);
    m->pooled = m->dalloc<float>(B * D); m->feat = m->dalloc<float>(B * D);
    m->out_f32 = m->dalloc<float>(B * D); m->out_f16 = m->dalloc<uint16_t>(B * D);
    bool ok = m->tokens_dev && m->x && m->h && m->dlt && m->kparts && m->mlp_h && m->qb && m->kb && m->vtb && m->pooled && m->feat && m->out_f32 && m->out_f16;
    ok = ok && fused_alloc_ok;
    for (auto& kv : m->slots) ok = ok && kv.second.dst;
    if (!ok) { mse_siglip_text_destroy(m); fail("siglip text: device allocation failed"); return nullptr; }
    (void)hipDeviceSynchronize();   // the zero fills above ran on the null stream; m->stream does not wait for it
    if (launch_vt_ones_row(m->vtb, BH + 4 * m->H, m->dh, m->dv_pad, m->n_pad, m->stream) || hipStreamSynchronize(m->stream) != hipSuccess) {
        mse_siglip_text_destroy(m);
        return nullptr;
    }
    return m;
}

void mse_siglip_text_destroy(mse_siglip_text* m) {
    if (!m) return;
    for (int hlf = 0; hlf < mse_siglip_text::MAX_PARTS; hlf++) {
        if (m->side[hlf]) { (void)hipStreamSynchronize(m->side[hlf]); (void)hipStreamDestroy(m->side[hlf]); }
        for (hipEvent_t e : m->side_ev[hlf]) if (e) (void)hipEventDestroy(e);
        if (m->part_s[hlf]) { (void)hipStreamSynchronize(m->part_s[hlf]); (void)hipStreamDestroy(m->part_s[hlf]); }
        if (m->part_join[hlf]) (void)hipEventDestroy(m->part_join[hlf]);
    }
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->stream) { (void)hipStreamSynchronize(m->stream); (void)hipStreamDestroy(m->stream); }
    delete m;   // frees the device memory
}

int mse_siglip_text_n_weights(const mse_siglip_text* m) { return m ? m->n_weights() : 0; }
const char* mse_siglip_text_weight_name(const mse_siglip_text* m, int idx) { return m ? m->weight_name(idx) : nullptr; }

int mse_siglip_text_set_weight(mse_siglip_text* m, const char* name, const float* data, const size_t* shape, int ndim) {
    if (!m || !name || !data) return fail("siglip_text_set_weight: null argument");
    return m->set_weight(name, data, shape, ndim);
}

int mse_siglip_text_finalize(mse_siglip_text* m) {
    if (!m) return fail("null engine");
    if (m->check_loaded() || m->fold_layernorms()) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(m->stream));
    m->finalized = true;
    return 0;
}

}  // extern "C"

// every kernel of one forward, enqueued on the engine's stream (and its part streams, joined back): tokens up, features into
// m->out_f32 / m->out_f16 on the device.  Nothing is copied back and nothing is waited for.
static int text_forward(mse_siglip_text* m, const int64_t* tokens, int batch, int normalize) {
    hipStream_t st = m->stream;
    const mse_siglip_text_config& c = m->cfg;
    const int D = m->D, T = m->ctx, M = batch * T;
    MSE_HIP_TRY(hipMemcpyAsync(m->tokens_dev, tokens, (size_t)M * 8, hipMemcpyHostToDevice, st));
    if (launch_embed_tokens(m->tokens_dev, m->tok_emb, m->pos, c.vocab_size, T, D, M, m->x, st)) return -1;
    // The blocks over the sequences [b0, b0 + nb) on stream `ss`.  b0 * T is a multiple of 256, so the GEMMs' row padding stays
    // inside the range's own rows (or behind the last range).
    // Up to 12 texts (768 rows): fc2 (K = 4352 for 1152 columns) is split four ways along K across workgroups, its partial sums and
    // bias added by the LayerNorm that consumes the branch (siglip_kernels.hip gemm_small_ksplit).  Such a call is one range of rows.
    BlockRun run;
    run.tokens = T; run.skinny = 1; run.n_branch = D; run.ld_branch = D;
    run.ksp_fc2 = gemm_small_ksplit(M, D, m->mlp_pad);
    run.ksp_proj = gemm_small_ksplit_short(M, D, D);   // the output projection of ONE text (the slabs share fc2's buffer: consumed in turn)
    run.kpart_stride = (size_t)gemm_small_ksplit_rows(M) * D;
    run.ln_wg = (size_t)M <= LN_WG_MAX_ROWS;   // by the CALL's rows (up to 16 texts): every part of a larger call runs layernorm_kernel
    // parts of a large batch (decided here because the fused path is chosen by the size of a part, the same for every part of a call)
    const int parts = batch >= 32 ? std::min(m->n_parts, batch / 16) : 1;
    const int per = parts > 1 ? std::max(4, (batch / parts) / 4 * 4) : batch;
    run.fused = m->fused && c.layers > 0 && per * T > FUSED_MIN_ROWS;
    LnDelta last;   // the last block's branch as the main stream's range (sequences 0 ..) left it
    auto blocks = [&](int b0, int nb, hipStream_t ss, int part) -> int {
        BlockRun r = run;
        r.b0 = b0; r.nb = nb;
        // large parts: the remainder launches of the N = 1152 / 3456 GEMMs beside their full column tiles (32-64 workgroups that ran
        // alone for 43 us after the 56 us of the four full tiles)
        r.side = nb * T > 512 ? m->side[part] : nullptr;
        r.side_fork = m->side_ev[part][0]; r.side_join = m->side_ev[part][1];
        LnDelta d;
        if (run_blocks(*m, r, ss, &d)) return -1;
        if (part == 0) last = d;
        return 0;
    };
    // A large batch runs as TWO halves on two streams (round 5, as the image tower does since round 2): the output-projection and fc2
    // GEMMs have 4.5 column tiles, so their last round of 256 x 256 tiles leaves most of the chip idle -- the other half's next kernel
    // takes those CUs.  The first half is a multiple of four sequences (256 rows).
    // (MSE_SIGLIP_TEXT_PARTS, read when the engine is created: 1..4 parts; every part but the last is a multiple of four sequences.)
    std::vector<SideRange> sides;
    for (int pt = 1; pt < parts; pt++) sides.push_back(SideRange{pt * per, pt + 1 == parts ? batch - pt * per : per, m->part_s[pt], m->part_join[pt]});
    if (fork_join(st, m->ev_fork, sides, parts > 1 ? per : batch, blocks)) return -1;
    // final LayerNorm of the LAST position only (pool_type "last": one row per text, the workgroup-per-row kernel at every batch), then
    // the projection with bias
    {
        LnDelta df;   // rows b * T + (T - 1): row stride T * D of x, of the bf16 branch and of the partial sums alike
        if (last.parts) { df = last; df.parts += (size_t)(T - 1) * D; df.ldp = T * D; }
        else if (last.bf16) { df.bf16 = last.bf16 + (size_t)(T - 1) * D; df.ldd = T * D; }
        if (launch_layernorm_d(m->x + (size_t)(T - 1) * D, 1, T * D, df, m->lnf_g, m->lnf_b, c.eps, D, batch, nullptr, D, m->pooled, 1, st)) return -1;
    }
    if (launch_small_linear(m->pooled, D, m->wproj, D, m->bproj, D, D, batch, m->feat, D, st)) return -1;
    if (launch_l2norm(m->feat, D, D, batch, normalize, m->out_f32, m->out_f16, st)) return -1;
    return 0;
}

extern "C" {

int mse_siglip_text_encode(mse_siglip_text* m, const int64_t* tokens, int batch, int normalize, float* out_f32, uint16_t* out_f16) {
    if (!m || !tokens) return fail("siglip text: null engine or tokens");
    if (!m->finalized) return fail("siglip text: call mse_siglip_text_finalize after loading the weights");
    std::lock_guard<std::mutex> call_lock(m->call_mu);
    if (batch <= 0 || batch > m->max_batch) return fail("siglip text: batch exceeds max_batch");  // clip_server.py:136
    if (text_forward(m, tokens, batch, normalize)) return -1;
    hipStream_t st = m->stream;
    const int D = m->D;
    if (out_f32) MSE_HIP_TRY(hipMemcpyAsync(out_f32, m->out_f32, (size_t)batch * D * 4, hipMemcpyDeviceToHost, st));
    if (out_f16) MSE_HIP_TRY(hipMemcpyAsync(out_f16, m->out_f16, (size_t)batch * D * 2, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// The same forward with the features LEFT ON THE DEVICE and no wait: the query path hands them to the search without a host round
// trip (src/query_disk_index.rs:345-381 embeds the text, :436-540 searches with it).  `tokens` must stay valid until the engine's
// stream has consumed them (pinned memory, or wait for the stream before reusing the buffer); the result buffers are the engine's
// own and hold this call's rows until the next call on the engine.
int mse_siglip_text_encode_dev(mse_siglip_text* m, const int64_t* tokens, int batch, int normalize) {
    if (!m || !tokens) return fail("siglip text: null engine or tokens");
    if (!m->finalized) return fail("siglip text: call mse_siglip_text_finalize after loading the weights");
    std::lock_guard<std::mutex> call_lock(m->call_mu);
    if (batch <= 0 || batch > m->max_batch) return fail("siglip text: batch exceeds max_batch");
    return text_forward(m, tokens, batch, normalize);
}
const void* mse_siglip_text_output_device(const mse_siglip_text* m, int which) {
    return m ? (which ? (const void*)m->out_f16 : (const void*)m->out_f32) : nullptr;
}
void* mse_siglip_text_stream(const mse_siglip_text* m) { return m ? (void*)m->stream : nullptr; }

}  // extern "C"
