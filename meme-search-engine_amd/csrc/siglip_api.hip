// C ABI of the SigLIP image engine: the in-process seam the reference fills with its AITemplate engines,
// `fast_image_fns[batch](images NCHW fp16 on device) -> [batch, 1152]` (clip_server.py:31,66-82,105-112),
// followed by the L2 normalisation and fp16 serialisation of do_inference / run_inference
// (clip_server.py:115,166).  Weights are addressed by the timm state-dict names the reference's loader maps
// (clip_server.py:40-57, without the "visual." prefix).
#include "../../include/mse.h"
#include "runtime.h"
#include "siglip_encoder.h"
#include "resize.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace mse;
using namespace mse::siglip;

// Geometry, weight store, blocks and their activations: Encoder (siglip_encoder.h); here what only the image tower has
struct mse_siglip : Encoder {
    mse_siglip_config cfg{};
    int tokens = 0, kpe = 0, kpe_pad = 0;
    // one call at a time per engine: a call enqueues its uploads and kernels on the engine's streams into shared scratch, so two
    // threads inside one engine would read each other's images (replicas are separate engines and run side by side)
    std::recursive_mutex call_mu;
    static constexpr int MAX_SIDE = 3;
    static constexpr int SMALL_BATCH = 4;   // images per call that still take the small-batch GEMM kernels (4 x 736 rows <= 3072)
    hipStream_t side[MAX_SIDE] = {};   // further streams of a forward pass (MSE_SIGLIP_STREAMS = 1 + how many are used; default 2)
    hipEvent_t ev_fork = nullptr, ev_join[MAX_SIDE] = {};
    int n_side = 0;
    // parameters
    uint16_t* wpe = nullptr; float* bpe = nullptr; float* pos = nullptr;
    float *lnf_g = nullptr, *lnf_b = nullptr;
    float* latent = nullptr; uint16_t *wq = nullptr, *wkv = nullptr, *wpp = nullptr, *wp1 = nullptr, *wp2 = nullptr;
    float *bq = nullptr, *bkv = nullptr, *bpp = nullptr, *lnp_g = nullptr, *lnp_b = nullptr, *bp1 = nullptr, *bp2 = nullptr;
    float* qlat = nullptr;
    // activations
    void* img_dev = nullptr;
    uint16_t *patches = nullptr, *kvb = nullptr;
    float *pool_a = nullptr, *pool_o = nullptr;
    uint16_t *pool_a16 = nullptr, *pool_ln16 = nullptr, *pool_h16 = nullptr;   // bf16 operands of the MAP head's GEMMs, rows padded to 256
    size_t pool_rows = 0;
    float* out_f32 = nullptr; uint16_t* out_f16 = nullptr;
    int last_batch = 0;
    bool no_small = false;       // MSE_SIGLIP_NOSMALL=1: calls of 1..4 images run the batch kernels too (bit-equal to rows of larger batches)
    std::shared_ptr<mse::resize::Context> resize_ctx;   // staging and tables of the device resize in front of the tower (resize_api.hip)
};

// what resize_api.hip needs of an engine: it fills img_dev on the engine's stream, under the engine's lock, then calls the forward pass
mse::resize::TowerInput mse::resize::tower_input(mse_siglip* m) {
    return TowerInput{&m->call_mu, m->stream, m->img_dev, m->cfg.img_size, m->cfg.in_chans, m->max_batch, m->finalized, &m->resize_ctx};
}

extern "C" {

mse_siglip* mse_siglip_create(const mse_siglip_config* c) {
    if (!c) { fail("null config"); return nullptr; }
    // 384 / 14 = 27 patches per side: the stride-14 convolution simply ignores the last 6 pixels
    if (c->emb_dim % 128 || c->num_heads <= 0 || c->emb_dim / c->num_heads != 72 || c->patch_size <= 0 ||
        c->img_size < c->patch_size || c->max_batch <= 0) {
        fail("siglip: unsupported geometry (emb_dim % 128 == 0, head_dim == 72 required)");
        return nullptr;
    }
    mse_siglip* m = new (std::nothrow) mse_siglip();
    if (!m) { fail("out of host memory"); return nullptr; }
    m->cfg = *c;
    m->what = "siglip"; m->eps = c->eps; m->gelu_tanh = c->gelu_tanh;
    const int g = c->img_size / c->patch_size;
    m->tokens = g * g; m->D = c->emb_dim; m->H = c->num_heads; m->dh = m->D / m->H; m->mlp = c->mlp_dim;
    m->mlp_pad = (int)round_up(m->mlp, 128);
    m->kpe = c->in_chans * c->patch_size * c->patch_size; m->kpe_pad = (int)round_up(m->kpe, 64);
    m->n_pad = (int)round_up(m->tokens, 32);
    m->max_batch = c->max_batch;
    // token rows of image b are rows b * n_pad + t of every [M][..] buffer: images start on 32-row boundaries, so
    // 8- and 16-token pieces never straddle two images (the transposed V scatter of the QKV epilogue needs that)
    m->m_pad = round_up((size_t)m->max_batch * m->n_pad, 256);
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { delete m; fail("hipStreamCreate failed"); return nullptr; }
    {
        const char* e = getenv("MSE_SIGLIP_STREAMS");
        m->n_side = std::min(std::max((e ? atoi(e) : 2) - 1, 0), (int)mse_siglip::MAX_SIDE);
        bool ok = m->n_side == 0 || hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < m->n_side; i++)
            ok = hipStreamCreateWithFlags(&m->side[i], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&m->ev_join[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) { mse_siglip_destroy(m); fail("hipStreamCreate failed"); return nullptr; }
    }
    const size_t D = m->D, MP = m->mlp_pad, DP = round_up(D, 256);
    m->dp = (int)DP;
    // parameters (names: clip_server.py:40-57)
    m->add_bf16("trunk.patch_embed.proj.weight", &m->wpe, D, m->kpe, D, m->kpe_pad);
    m->add_f32("trunk.patch_embed.proj.bias", &m->bpe, 1, D);
    m->pos = m->dalloc<float>((size_t)m->n_pad * D, true);   // padded to the row stride (EPI_PATCH indexes it by m % n_pad)
    m->slots["trunk.pos_embed"] = Slot{false, m->pos, (size_t)m->tokens, D, (size_t)m->tokens, D};
    m->add_blocks(c->depth, BlockNames{"trunk.blocks.", "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias",
                                       "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight",
                                       "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"});
    {
        const char* e = getenv("MSE_SIGLIP_NOSMALL");
        m->no_small = e && atoi(e);
    }
    {
        const char* e = getenv("MSE_SIGLIP_NOFUSE");
        m->fused = !(e && atoi(e)) && gemm_fused_ok((int)m->m_pad, (int)D, (int)MP, m->H, m->dh, m->n_pad, m->n_pad, 8);
    }
    const bool fused_alloc_ok = !m->fused || m->alloc_fused();
    m->add_f32("trunk.norm.weight", &m->lnf_g, 1, D); m->add_f32("trunk.norm.bias", &m->lnf_b, 1, D);
    const std::string ap = "trunk.attn_pool.";
    m->add_f32(ap + "latent", &m->latent, 1, D);
    m->add_bf16(ap + "q.weight", &m->wq, D, D, D, D); m->add_f32(ap + "q.bias", &m->bq, 1, D);
    m->add_bf16(ap + "kv.weight", &m->wkv, 2 * D, D, 2 * D, D); m->add_f32(ap + "kv.bias", &m->bkv, 1, 2 * D);
    m->add_bf16(ap + "proj.weight", &m->wpp, D, D, D, D); m->add_f32(ap + "proj.bias", &m->bpp, 1, D);
    m->add_f32(ap + "norm.weight", &m->lnp_g, 1, D); m->add_f32(ap + "norm.bias", &m->lnp_b, 1, D);
    m->add_bf16(ap + "mlp.fc1.weight", &m->wp1, m->mlp, D, MP, D); m->add_f32(ap + "mlp.fc1.bias", &m->bp1, 1, m->mlp, MP);
    m->add_bf16(ap + "mlp.fc2.weight", &m->wp2, D, m->mlp, D, MP); m->add_f32(ap + "mlp.fc2.bias", &m->bp2, 1, D);
    // activations
    const size_t B = m->max_batch, M = m->m_pad, BH = B * m->H;
    m->img_dev = m->dalloc<float>(B * c->in_chans * c->img_size * c->img_size);
    m->patches = m->dalloc<uint16_t>(M * m->kpe_pad, true);
    m->x = m->dalloc<uint16_t>(M * D, true);   // residual stream, fp16
    m->h = m->dalloc<uint16_t>(M * D, true);
    m->dlt = m->dalloc<uint16_t>(M * DP, true);
    m->mlp_h = m->dalloc<uint16_t>(M * MP, true);
    m->qb = m->dalloc<uint16_t>((BH + m->H) * m->n_pad * m->dh_pad, true);   // one image of slack (rows of the M padding)
    m->kb = m->dalloc<uint16_t>((BH + m->H) * m->n_pad * attention_k_stride(), true);   // 224-byte rows (attention DMA)
    m->vtb = m->dalloc<uint16_t>((BH + m->H) * m->dv_pad * m->n_pad, true);
    m->kvb = m->dalloc<uint16_t>(M * 2 * D, true);
    m->qlat = m->dalloc<float>(D, true);
    m->kparts = m->dalloc<float>((size_t)4 * 768 * D, true);   // K-split partial sums of fc2 for ONE image (4 ranges x 768 rows)
    m->pool_rows = round_up(B, 256);
    m->pool_a = m->dalloc<float>(B * D); m->pool_o = m->dalloc<float>(m->pool_rows * D, true);
    m->pool_a16 = m->dalloc<uint16_t>(m->pool_rows * D, true); m->pool_ln16 = m->dalloc<uint16_t>(m->pool_rows * D, true);
    m->pool_h16 = m->dalloc<uint16_t>(m->pool_rows * MP, true);
    m->out_f32 = m->dalloc<float>(B * D); m->out_f16 = m->dalloc<uint16_t>(B * D);
    bool ok = m->img_dev && m->patches && m->x && m->h && m->dlt && m->mlp_h && m->qb && m->kb && m->vtb && m->kvb && m->qlat && m->kparts &&
              m->pool_a && m->pool_o && m->pool_a16 && m->pool_ln16 && m->pool_h16 && m->out_f32 && m->out_f16;
    ok = ok && fused_alloc_ok;
    for (auto& kv : m->slots) ok = ok && kv.second.dst;
    if (!ok) { mse_siglip_destroy(m); fail("siglip: device allocation failed"); return nullptr; }
    (void)hipDeviceSynchronize();   // the zero fills above ran on the null stream; m->stream does not wait for it
    if (launch_vt_ones_row(m->vtb, BH + m->H, m->dh, m->dv_pad, m->n_pad, m->stream) || hipStreamSynchronize(m->stream) != hipSuccess) {
        mse_siglip_destroy(m);
        return nullptr;
    }
    return m;
}

void mse_siglip_destroy(mse_siglip* m) {
    if (!m) return;
    for (int i = 0; i < mse_siglip::MAX_SIDE; i++) {
        if (m->side[i]) { (void)hipStreamSynchronize(m->side[i]); (void)hipStreamDestroy(m->side[i]); }
        if (m->ev_join[i]) (void)hipEventDestroy(m->ev_join[i]);
    }
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->stream) { (void)hipStreamSynchronize(m->stream); (void)hipStreamDestroy(m->stream); }
    delete m;   // frees the device memory
}

int mse_siglip_n_weights(const mse_siglip* m) { return m ? m->n_weights() : 0; }

// name of weight #idx (sorted), or NULL; lets a loader enumerate what the engine expects
const char* mse_siglip_weight_name(const mse_siglip* m, int idx) { return m ? m->weight_name(idx) : nullptr; }

int mse_siglip_set_weight(mse_siglip* m, const char* name, const float* data, const size_t* shape, int ndim) {
    if (!m || !name || !data) return fail("siglip_set_weight: null argument");
    return m->set_weight(name, data, shape, ndim);
}

int mse_siglip_finalize(mse_siglip* m) {
    if (!m) return fail("null engine");
    if (m->check_loaded()) return -1;
    // the pooling query does not depend on the input: q = Linear(latent)   (model.py:94-95)
    if (launch_small_linear(m->latent, m->D, m->wq, m->D, m->bq, m->D, m->D, 1, m->qlat, m->D, m->stream)) return -1;
    if (m->fold_layernorms()) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(m->stream));
    m->finalized = true;
    return 0;
}

// Decoded RGB bytes in, features out: the ToTensor / Normalize / .half() / stack / H2D steps of the reference's
// preprocessing thread (clip_server.py:131-146) run on the device, and the PCIe copy is the u8 image (1 B/element)
int mse_siglip_encode_rgb8(mse_siglip* m, const uint8_t* rgb_hwc, int batch, int normalize, float* out_f32, uint16_t* out_f16) {
    if (!m || !rgb_hwc) return fail("null engine or image");
    std::lock_guard<std::recursive_mutex> call_lock(m->call_mu);
    if (batch <= 0 || batch > m->max_batch) return fail("siglip: batch exceeds max_batch");
    const mse_siglip_config& c = m->cfg;
    const size_t elems = (size_t)batch * c.in_chans * c.img_size * c.img_size;
    uint8_t* u8 = reinterpret_cast<uint8_t*>(m->img_dev) + 2 * (size_t)m->max_batch * c.in_chans * c.img_size * c.img_size;
    MSE_HIP_TRY(hipMemcpyAsync(u8, rgb_hwc, elems, hipMemcpyHostToDevice, m->stream));
    if (launch_rgb8_to_nchw_f16(u8, m->img_dev, batch, c.in_chans, c.img_size, c.img_size, m->stream)) return -1;
    return mse_siglip_encode_image(m, m->img_dev, 1, 1, batch, normalize, out_f32, out_f16);
}

// BITMAPFILEHEADER (14 bytes) + BITMAPINFOHEADER or one of its longer successors: what `image::codecs::bmp::BmpEncoder`
// writes for Rgb8 (54-byte header, bottom-up rows) and what PIL writes.  Anything else (palettes, RLE, 32 bits, OS/2 headers)
// is not "plain" and goes through the host decoder instead.
int mse_bmp24_info(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height, uint32_t* pixel_offset, int* bottom_up) {
    auto u16 = [&](size_t o) { return (uint32_t)data[o] | ((uint32_t)data[o + 1] << 8); };
    auto u32 = [&](size_t o) { return u16(o) | (u16(o + 2) << 16); };
    if (!data || size < 54 || data[0] != 'B' || data[1] != 'M') return fail("not a BMP file");
    const uint32_t off = u32(10), dib = u32(14);
    if (dib < 40 || 14 + (size_t)dib > size) return fail("BMP: unsupported header");
    const int32_t w = (int32_t)u32(18), h = (int32_t)u32(22);
    if (u16(26) != 1 || u16(28) != 24 || u32(30) != 0) return fail("BMP: not uncompressed 24-bit");
    if (w <= 0 || h == 0 || w > 65535 || h > 65535 || h < -65535) return fail("BMP: bad dimensions");
    const uint32_t ah = (uint32_t)(h < 0 ? -h : h);
    const size_t stride = ((size_t)w * 3 + 3) & ~(size_t)3;
    if (off < 14 + dib || (size_t)off + stride * ah > size) return fail("BMP: pixel array exceeds the file");
    if (width) *width = (uint32_t)w;
    if (height) *height = ah;
    if (pixel_offset) *pixel_offset = off;
    if (bottom_up) *bottom_up = h > 0;
    return 0;
}

// Request bytes in, features out: header check on the host (54 bytes), the pixel arrays go up as they are and the device does
// BGR -> RGB, the row flip, ToTensor / Normalize / .half() (the whole of clip_server.py:131-146 for the client's own format).
int mse_siglip_encode_bmp(mse_siglip* m, const uint8_t* const* bmps, const size_t* sizes, int batch, int normalize, float* out_f32,
                          uint16_t* out_f16) {
    if (!m || !bmps || !sizes) return fail("null engine or image list");
    std::lock_guard<std::recursive_mutex> call_lock(m->call_mu);
    if (batch <= 0 || batch > m->max_batch) return fail("siglip: batch exceeds max_batch");
    const mse_siglip_config& c = m->cfg;
    if (c.in_chans != 3) return fail("siglip: BMP input needs a 3-channel model");
    const int S = c.img_size;
    const size_t row_stride = ((size_t)S * 3 + 3) & ~(size_t)3, img_stride = row_stride * S;
    // staging: behind the fp16 image (2 bytes per element of a 4-byte-per-element allocation), flags after the pixels
    uint8_t* u8 = reinterpret_cast<uint8_t*>(m->img_dev) + 2 * (size_t)m->max_batch * 3 * S * S;
    const size_t room = 2 * (size_t)m->max_batch * 3 * S * S;
    if ((size_t)batch * img_stride + batch > room) return fail("siglip: BMP staging does not fit");
    std::vector<uint8_t> flags(batch);
    for (int b = 0; b < batch; b++) {
        uint32_t w = 0, h = 0, off = 0;
        int bu = 0;
        if (mse_bmp24_info(bmps[b], sizes[b], &w, &h, &off, &bu)) return -1;
        if ((int)w != S || (int)h != S) return fail("BMP: image is not " + std::to_string(S) + " x " + std::to_string(S));
        flags[b] = (uint8_t)bu;
        MSE_HIP_TRY(hipMemcpyAsync(u8 + (size_t)b * img_stride, bmps[b] + off, img_stride, hipMemcpyHostToDevice, m->stream));
    }
    uint8_t* flags_dev = u8 + (size_t)batch * img_stride;
    MSE_HIP_TRY(hipMemcpyAsync(flags_dev, flags.data(), batch, hipMemcpyHostToDevice, m->stream));
    MSE_HIP_TRY(hipStreamSynchronize(m->stream));   // `flags` is a stack-owned source
    if (launch_bmp24_to_nchw_f16(u8, img_stride, (int)row_stride, flags_dev, m->img_dev, batch, S, S, m->stream)) return -1;
    return mse_siglip_encode_image(m, m->img_dev, 1, 1, batch, normalize, out_f32, out_f16);
}

int mse_siglip_encode_image(mse_siglip* m, const void* images, int dtype, int on_device, int batch, int normalize,
                            float* out_f32, uint16_t* out_f16) {
    if (!m) return fail("null engine");
    if (!m->finalized) return fail("siglip: call mse_siglip_finalize after loading the weights");
    std::lock_guard<std::recursive_mutex> call_lock(m->call_mu);
    if (batch <= 0 || batch > m->max_batch) return fail("siglip: batch exceeds max_batch");  // clip_server.py:139
    if (dtype != 0 && dtype != 1) return fail("siglip: dtype must be 0 (f32) or 1 (f16)");
    hipStream_t st = m->stream;
    const mse_siglip_config& c = m->cfg;
    const size_t img_elems = (size_t)batch * c.in_chans * c.img_size * c.img_size;
    const void* img = images;
    if (!on_device) {
        MSE_HIP_TRY(hipMemcpyAsync(m->img_dev, images, img_elems * (dtype ? 2 : 4), hipMemcpyHostToDevice, st));
        img = m->img_dev;
    }
    const int D = m->D, T = m->tokens, TS = m->n_pad, DP = m->dp;
    const int gelu_tanh = c.gelu_tanh;
    const size_t img_stride = (size_t)c.in_chans * c.img_size * c.img_size * (dtype ? 2 : 4);
    // The trunk (patch embedding .. MAP-head pooling) of images [b0, b0 + batch) on stream st: every activation buffer is indexed by
    // image or by token row b * n_pad + t, so a sub-batch that starts at a multiple of 8 images (= 23 whole 256-row blocks) is just
    // an offset into each of them.
    // Up to SMALL_BATCH images (<= 3072 token rows) take the small-batch GEMM kernels (siglip_kernels.hip "Mid-size GEMM") with
    // LayerNorm as a pass of its own: the 256-row tiles of the batch kernels put 15-200 workgroups on 256 CUs (7.6 ms for ONE image,
    // 3.3 with these).  Decided by the CALL's batch, so every row of a larger batch still runs the same arithmetic whatever its
    // sub-batch; an image encoded alone agrees with the same image inside a batch of more than SMALL_BATCH to bf16 rounding (both
    // within the oracle's tolerance), not bit for bit.  MSE_SIGLIP_NOSMALL=1 (read when the engine is created) keeps the batch kernels
    // for every size.
    const int sk = (!m->no_small && batch <= mse_siglip::SMALL_BATCH) ? 1 : 0;
    // The LayerNorm kernel of the trunk, also by the CALL: the workgroup-per-row kernel for a small call of at most LN_WG_MAX_ROWS
    // token rows (ONE image), layernorm_kernel for everything else -- a trailing sub-batch of one image and a one-image call under
    // MSE_SIGLIP_NOSMALL=1 included, whose rows must equal those of any larger batch bit for bit.
    const int ln_wg = sk && (size_t)batch * TS <= LN_WG_MAX_ROWS;
    auto trunk = [&](int b0, int batch, hipStream_t st, int) -> int {
        const size_t r0 = (size_t)b0 * TS;
        const void* v_img = reinterpret_cast<const char*>(img) + (size_t)b0 * img_stride;
        uint16_t* v_patches = m->patches + r0 * m->kpe_pad;
        uint16_t *v_x = m->x + r0 * D, *v_h = m->h + r0 * D, *v_kvb = m->kvb + r0 * 2 * D;
        float* v_pool_a = m->pool_a + (size_t)b0 * D;
        const int M = batch * TS;   // rows incl. the (finite, never read as keys) padding rows of every image
        const int Mp = (int)round_up(M, 256);
        // PatchEmbedder + PositionalEmbeddings (model.py:57-80,122)
        if (launch_patchify(v_img, dtype, batch, c.in_chans, c.img_size, c.img_size, c.patch_size, m->kpe_pad, TS, v_patches, st)) return -1;
        {
            GemmLaunch g; g.x = v_patches; g.w = m->wpe; g.bias = m->bpe; g.M = Mp; g.N = D; g.K = m->kpe_pad; g.m_valid = M;
            g.out_bf16 = v_x; g.ldo = D; g.ldr = D; g.pos = m->pos; g.tokens = TS;   // writes the fp16 residual stream
            g.skinny = sk;
            if (launch_gemm(GEMM_EPI_PATCH, g, st)) return -1;
        }
        BlockRun r; r.b0 = b0; r.nb = batch; r.tokens = T; r.skinny = sk; r.ln_wg = ln_wg;
        r.fused = !sk && m->fused && gemm_fused_ok(Mp, D, m->mlp_pad, m->H, m->dh, TS, m->n_pad, M);
        r.n_branch = sk ? D : DP; r.ld_branch = DP;   // columns >= D of the branch are padding
        // one image: fc2 (K = 4352 for 1152 columns) is split four ways along K across workgroups; its partial sums and bias are added
        // by the LayerNorm that consumes the branch (siglip_kernels.hip gemm_small_ksplit)
        r.ksp_fc2 = sk ? gemm_small_ksplit(M, D, m->mlp_pad) : 1;
        r.kpart_stride = (size_t)gemm_small_ksplit_rows(M) * D;
        LnDelta df;   // what the final LayerNorm adds to x
        if (run_blocks(*m, r, st, &df)) return -1;
        if (launch_layernorm_d(v_x, 1, D, df, m->lnf_g, m->lnf_b, c.eps, D, M, v_h, D, nullptr, ln_wg, st)) return -1;  // model.py:50,55
        // MAPHead (model.py:82-111)
        {
            GemmLaunch g; g.x = v_h; g.w = m->wkv; g.bias = m->bkv; g.M = Mp; g.N = 2 * D; g.K = D; g.m_valid = M;
            g.out_bf16 = v_kvb; g.ldo = 2 * D; g.skinny = sk;
            if (launch_gemm(GEMM_EPI_BF16, g, st)) return -1;
        }
        if (launch_pool_attention(v_kvb, 2 * D, m->qlat, batch, m->H, m->dh, T, TS, v_pool_a, D, st)) return -1;
        return 0;
    };
    // Sub-batches on separate streams: a persistent GEMM's last round leaves most CUs idle (736 row blocks over 256 CUs), and another
    // sub-batch's next kernel takes them.  MSE_SIGLIP_STREAMS=1 keeps the whole batch on one stream.
    const int parts = std::min(m->n_side + 1, batch / 16);
    const int per = parts > 1 ? (int)round_up((size_t)(batch + parts - 1) / parts, 8) : batch;
    std::vector<SideRange> sides;
    for (int b0 = per; parts > 1 && b0 < batch; b0 += per)
        sides.push_back(SideRange{b0, std::min(per, batch - b0), m->side[sides.size()], m->ev_join[sides.size()]});
    if (fork_join(st, m->ev_fork, sides, sides.empty() ? batch : per, trunk)) return -1;
    // proj, LayerNorm, MLP with residual on the matrix cores: the batch is one (or a few) 256-row block of the same GEMM kernels
    // (rows >= batch are zero padding; the fp32 accumulating epilogue builds pool_o = proj, then pool_o += fc2)
    {
        const int Bp = (int)round_up((size_t)batch, 256);
        if (launch_f32_to_bf16_pad(m->pool_a, batch, D, D, m->pool_a16, Bp, D, st)) return -1;
        MSE_HIP_TRY(hipMemsetAsync(m->pool_o, 0, (size_t)Bp * D * 4, st));
        GemmLaunch g; g.x = m->pool_a16; g.w = m->wpp; g.bias = m->bpp; g.M = Bp; g.N = D; g.K = D; g.m_valid = batch;
        g.resid = m->pool_o; g.ldr = D; g.skinny = sk;
        if (launch_gemm(GEMM_EPI_RESID, g, st)) return -1;
        // (one pooled row per image: the workgroup-per-row kernel at EVERY batch, so a row never changes with the batch around it)
        if (launch_layernorm(m->pool_o, 0, D, nullptr, 0, m->lnp_g, m->lnp_b, c.eps, D, batch, m->pool_ln16, D, nullptr, 1, st)) return -1;
        GemmLaunch g1; g1.x = m->pool_ln16; g1.w = m->wp1; g1.bias = m->bp1; g1.M = Bp; g1.N = m->mlp_pad; g1.K = D; g1.m_valid = batch;
        g1.out_bf16 = m->pool_h16; g1.ldo = m->mlp_pad; g1.gelu_tanh = gelu_tanh; g1.skinny = sk;
        if (launch_gemm(GEMM_EPI_GELU, g1, st)) return -1;
        GemmLaunch g2; g2.x = m->pool_h16; g2.w = m->wp2; g2.bias = m->bp2; g2.M = Bp; g2.N = D; g2.K = m->mlp_pad; g2.m_valid = batch;
        g2.resid = m->pool_o; g2.ldr = D; g2.skinny = sk;
        if (launch_gemm(GEMM_EPI_RESID, g2, st)) return -1;
    }
    // features /= norm (clip_server.py:115); fp16 rows are what the server serialises (clip_server.py:166)
    if (launch_l2norm(m->pool_o, D, D, batch, normalize, m->out_f32, m->out_f16, st)) return -1;
    if (out_f32) MSE_HIP_TRY(hipMemcpyAsync(out_f32, m->out_f32, (size_t)batch * D * 4, hipMemcpyDeviceToHost, st));
    if (out_f16) MSE_HIP_TRY(hipMemcpyAsync(out_f16, m->out_f16, (size_t)batch * D * 2, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    m->last_batch = batch;
    return 0;
}

// device pointer to the [batch][emb] fp32 (which = 0) / fp16 (which = 1) result of the last call
const void* mse_siglip_output_device(const mse_siglip* m, int which) { return m ? (which ? (const void*)m->out_f16 : (const void*)m->out_f32) : nullptr; }

void* mse_siglip_stream(const mse_siglip* m) { return m ? (void*)m->stream : nullptr; }

// developer hook: average ms of the fc1-shaped GEMM (bias + GELU) over `iters` launches with ablation `abl`
namespace {
// developer data for the GEMM timing hook: bf16 values uniform in (-1, 1) from a counter hash (MSE_GEMM_RANDOM=1);
// constant operands let the chip clock higher than real activations do
__global__ void fill_random_bf16_kernel(uint16_t* p, size_t n, uint32_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t h = (uint32_t)i * 2654435761u + seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
        const float f = (float)(int32_t)h * (1.0f / 2147483648.0f);
        p[i] = (uint16_t)(__float_as_uint(f) >> 16);
    }
}
}  // namespace

int mse_debug_gemm_ms(int M, int N, int K, int abl, int iters, float* ms_out) {
    if (M % 256 || N % 256 || K % 64) return fail("debug gemm: M, N multiples of 256, K of 64");
    DevBuf x, w, bias, out;
    if (x.ensure((size_t)M * K * 2) || w.ensure((size_t)N * K * 2) || bias.ensure((size_t)N * 4) || out.ensure((size_t)M * N * 2)) return -1;
    MSE_HIP_TRY(hipMemset(x.p, 0x3c, (size_t)M * K * 2));   // bf16 0x3c3c ~ 0.0115
    MSE_HIP_TRY(hipMemset(w.p, 0x3c, (size_t)N * K * 2));
    MSE_HIP_TRY(hipMemset(bias.p, 0, (size_t)N * 4));
    if (MSE_DEV_KNOB("MSE_GEMM_RANDOM")) {   // developer library: operands with random mantissas
        hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(4096), dim3(256), 0, nullptr, x.as<uint16_t>(), (size_t)M * K, 1u);
        hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(4096), dim3(256), 0, nullptr, w.as<uint16_t>(), (size_t)N * K, 2u);
        MSE_HIP_TRY(hipGetLastError());
    }
    GemmLaunch g; g.x = x.as<uint16_t>(); g.w = w.as<uint16_t>(); g.bias = bias.as<float>(); g.M = M; g.N = N; g.K = K;
    g.m_valid = M; g.out_bf16 = out.as<uint16_t>(); g.ldo = N;
    hipEvent_t e0, e1;
    MSE_HIP_TRY(hipEventCreate(&e0)); MSE_HIP_TRY(hipEventCreate(&e1));
    if (launch_gemm256_ablation(abl, g, nullptr)) return -1;
    MSE_HIP_TRY(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; i++) if (launch_gemm256_ablation(abl, g, nullptr)) return -1;
    MSE_HIP_TRY(hipEventRecord(e1, nullptr));
    MSE_HIP_TRY(hipEventSynchronize(e1));
    float ms = 0; MSE_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

// developer / test hook for the small-batch GEMM kernels: `rows` real rows of a [rows][K] x [N][K]^T product with the bias (epi 0) or
// bias + GELU (epi 1) epilogue, run by `variant` (0 = the large-batch kernels, 1 = chosen by size, 2 = K-split skinny, 3 = 64 x 64
// tiles, 4 = 128 x 128 tiles).  ms_out: average over `iters` launches, each with its OWN weight matrix out of a ring larger than
// the last-level cache (weights stream from HBM in a forward pass); n_diff (optional, two words): output elements that differ from
// the large-batch kernels', and those that differ by more than two bf16 steps (must be 0: the kernels differ in summation order only).
int mse_debug_gemm_small(int rows, int N, int K, int epi, int variant, int iters, float* ms_out, uint64_t* n_diff) {
    if (rows <= 0 || N % 128 || K % 64 || iters <= 0 || (epi != 0 && epi != 1) || variant < 0 || variant > 4)
        return fail("debug gemm small: rows > 0, N % 128 == 0, K % 64 == 0, epi 0 / 1, variant 0..4");
    const int M = (int)round_up((size_t)rows, 256);
    const size_t wbytes = (size_t)N * K * 2;
    const int ring = (int)std::min<size_t>(64, std::max<size_t>(1, ((size_t)768 << 20) / wbytes));
    DevBuf x, w, bias, out, ref;
    if (x.ensure((size_t)M * K * 2) || w.ensure(wbytes * ring) || bias.ensure((size_t)N * 4) || out.ensure((size_t)M * N * 2) ||
        ref.ensure((size_t)M * N * 2)) return -1;
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(4096), dim3(256), 0, nullptr, x.as<uint16_t>(), (size_t)M * K, 1u);
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(4096), dim3(256), 0, nullptr, w.as<uint16_t>(), (size_t)N * K * ring, 2u);
    MSE_HIP_TRY(hipGetLastError());
    {
        std::vector<float> hb(N);
        for (int n = 0; n < N; n++) hb[n] = 0.01f * (float)((n * 37) % 101 - 50);
        MSE_HIP_TRY(hipMemcpy(bias.p, hb.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    }
    MSE_HIP_TRY(hipMemset(out.p, 0, (size_t)M * N * 2));
    MSE_HIP_TRY(hipMemset(ref.p, 0, (size_t)M * N * 2));
    auto run = [&](int var, int slot, uint16_t* dst) -> int {
        GemmLaunch g; g.x = x.as<uint16_t>(); g.w = w.as<uint16_t>() + (size_t)slot * N * K; g.bias = bias.as<float>();
        g.M = M; g.N = N; g.K = K; g.m_valid = rows; g.out_bf16 = dst; g.ldo = N; g.skinny = var;
        return launch_gemm(epi ? GEMM_EPI_GELU : GEMM_EPI_BF16, g, nullptr);
    };
    if (n_diff) {
        if (run(0, 0, ref.as<uint16_t>()) || run(variant, 0, out.as<uint16_t>())) return -1;
        MSE_HIP_TRY(hipDeviceSynchronize());
        std::vector<uint16_t> ha((size_t)M * N), hb((size_t)M * N);
        MSE_HIP_TRY(hipMemcpy(ha.data(), ref.p, ha.size() * 2, hipMemcpyDeviceToHost));
        MSE_HIP_TRY(hipMemcpy(hb.data(), out.p, hb.size() * 2, hipMemcpyDeviceToHost));
        uint64_t d = 0, far = 0;
        auto f = [](uint16_t h) { uint32_t u = (uint32_t)h << 16; float v; memcpy(&v, &u, 4); return v; };
        for (size_t r = 0; r < (size_t)rows; r++)
            for (size_t n = 0; n < (size_t)N; n++) {
                const uint16_t p = ha[r * N + n], q = hb[r * N + n];
                if (p == q) continue;
                d++;
                const float x = f(p), y = f(q);
                if (!(fabsf(x - y) <= 0.0157f * std::max(fabsf(x), fabsf(y)) + 1e-3f)) far++;   // more than two bf16 steps apart (or not finite)
            }
        n_diff[0] = d;
        n_diff[1] = far;
    }
    hipEvent_t e0, e1;
    MSE_HIP_TRY(hipEventCreate(&e0)); MSE_HIP_TRY(hipEventCreate(&e1));
    for (int i = 0; i < std::min(ring, 4); i++) if (run(variant, i, out.as<uint16_t>())) return -1;
    MSE_HIP_TRY(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; i++) if (run(variant, i % ring, out.as<uint16_t>())) return -1;
    MSE_HIP_TRY(hipEventRecord(e1, nullptr));
    MSE_HIP_TRY(hipEventSynchronize(e1));
    float ms = 0; MSE_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

namespace {
uint16_t host_bf16(float f) {   // round to nearest even (finite inputs)
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
float host_bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// finite garbage for the padding of the attention operands: bf16 values of magnitude up to 1e4 from a counter hash
uint16_t poison_bf16(size_t i, uint32_t seed) {
    uint32_t h = (uint32_t)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return host_bf16((float)(int32_t)h * (1.0e4f / 2147483648.0f));
}
constexpr int DBG_DH = 72, DBG_DH_PAD = 96, DBG_DV_PAD = 80;   // the towers' head geometry (Encoder: dh, dh_pad, dv_pad)
}  // namespace

// test hook for the self-attention launchers: q / k / v are host fp32 [B][heads][tokens][72], rounded here to bf16 (nearest even) and
// laid out as the QKV epilogue leaves them (q rows of 96, K rows of attention_k_stride(), Vt [80][n_pad], n_pad = tokens rounded up to
// 32, everything else zero); launch_vt_ones_row, then launch_attention exactly as run_blocks calls it, so the tiling is chosen from
// (B, heads, tokens) as in the towers.  out: host fp32 [B][tokens][heads * 72], the bf16 result widened.
// flags bit 0: fill the padding -- K rows, q rows and Vt columns (rows 0..71) tokens .. n_pad - 1 -- with finite garbage of magnitude
// up to 1e4 instead of zeros; the row-sum row stays ones.
// K and Vt carry `heads` further zeroed matrices like the engines' buffers (BH + H): with n_pad % 64 == 32 the kernel's last 64-key
// stage reads 32 K rows (7 KiB) past every matrix and 64 bytes past every Vt row, the last matrix's included.
int mse_debug_siglip_attention(const float* q, const float* k, const float* v, int B, int heads, int tokens, int flags, float* out) {
    if (!q || !k || !v || !out) return fail("debug siglip attention: null argument");
    if (B <= 0 || heads <= 0 || tokens <= 0 || (flags & ~1) || (size_t)B * heads * tokens > ((size_t)1 << 22))
        return fail("debug siglip attention: B, heads, tokens > 0, B * heads * tokens <= 2^22, flags 0 / 1");
    const size_t T = tokens, NP = round_up(T, 32), BH = (size_t)B * heads, KS = attention_k_stride();
    const size_t D = (size_t)heads * DBG_DH;
    std::vector<uint16_t> hq(BH * NP * DBG_DH_PAD, 0), hk((BH + heads) * NP * KS, 0), hvt((BH + heads) * DBG_DV_PAD * NP, 0);
    for (size_t bh = 0; bh < BH; bh++)
        for (size_t t = 0; t < NP; t++)
            for (size_t e = 0; e < (size_t)DBG_DH; e++) {
                const size_t qi = (bh * NP + t) * DBG_DH_PAD + e, ki = (bh * NP + t) * KS + e, vi = (bh * DBG_DV_PAD + e) * NP + t;
                if (t < T) {
                    const size_t src = (bh * T + t) * DBG_DH + e;
                    hq[qi] = host_bf16(q[src]); hk[ki] = host_bf16(k[src]); hvt[vi] = host_bf16(v[src]);
                } else if (flags & 1) {
                    hq[qi] = poison_bf16(qi, 0x51u); hk[ki] = poison_bf16(ki, 0x4bu); hvt[vi] = poison_bf16(vi, 0x56u);
                }
            }
    DevBuf dq, dk, dvt, dout;
    const size_t out_elems = (size_t)B * NP * D;
    if (dq.ensure(hq.size() * 2) || dk.ensure(hk.size() * 2) || dvt.ensure(hvt.size() * 2) || dout.ensure(out_elems * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(dq.p, hq.data(), hq.size() * 2, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(dk.p, hk.data(), hk.size() * 2, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(dvt.p, hvt.data(), hvt.size() * 2, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemset(dout.p, 0, out_elems * 2));
    if (launch_vt_ones_row(dvt.as<uint16_t>(), BH + heads, DBG_DH, DBG_DV_PAD, (int)NP, nullptr)) return -1;
    if (launch_attention(dq.as<uint16_t>(), dk.as<uint16_t>(), dvt.as<uint16_t>(), B, heads, tokens, (int)NP, DBG_DH, DBG_DH_PAD, DBG_DV_PAD,
                         dout.as<uint16_t>(), (int)D, (int)NP, nullptr)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    std::vector<uint16_t> ho(out_elems);
    MSE_HIP_TRY(hipMemcpy(ho.data(), dout.p, out_elems * 2, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < (size_t)B; b++)
        for (size_t t = 0; t < T; t++)
            for (size_t c = 0; c < D; c++) out[(b * T + t) * D + c] = host_bf16_to_f32(ho[(b * NP + t) * D + c]);
    return 0;
}

// test hook for the pooling attention (MAP head): qlat host fp32 [heads * 72] (used as it is, the kernel reads it in fp32); k / v host
// fp32 [B][tokens][heads * 72], rounded to bf16 and interleaved into the kv projection's layout ([B * n_pad][2 * D], k in columns
// [0, D), v in [D, 2D), padding rows zero); launch_pool_attention as the image tower calls it.  out: host fp32 [B][heads * 72].
int mse_debug_siglip_pool_attention(const float* qlat, const float* k, const float* v, int B, int heads, int tokens, float* out) {
    if (!qlat || !k || !v || !out) return fail("debug siglip pool attention: null argument");
    if (B <= 0 || heads <= 0 || tokens <= 0 || tokens > 8192 || (size_t)B * heads * tokens > ((size_t)1 << 22))
        return fail("debug siglip pool attention: B, heads > 0, 0 < tokens <= 8192, B * heads * tokens <= 2^22");
    const size_t T = tokens, NP = round_up(T, 32), D = (size_t)heads * DBG_DH;
    std::vector<uint16_t> hkv((size_t)B * NP * 2 * D, 0);
    for (size_t b = 0; b < (size_t)B; b++)
        for (size_t t = 0; t < T; t++)
            for (size_t c = 0; c < D; c++) {
                hkv[(b * NP + t) * 2 * D + c] = host_bf16(k[(b * T + t) * D + c]);
                hkv[(b * NP + t) * 2 * D + D + c] = host_bf16(v[(b * T + t) * D + c]);
            }
    DevBuf dkv, dql, dout;
    if (dkv.ensure(hkv.size() * 2) || dql.ensure(D * 4) || dout.ensure((size_t)B * D * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(dkv.p, hkv.data(), hkv.size() * 2, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(dql.p, qlat, D * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemset(dout.p, 0, (size_t)B * D * 4));
    if (launch_pool_attention(dkv.as<uint16_t>(), (int)(2 * D), dql.as<float>(), B, heads, DBG_DH, tokens, (int)NP, dout.as<float>(), (int)D,
                              nullptr)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    MSE_HIP_TRY(hipMemcpy(out, dout.p, (size_t)B * D * 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

namespace {
uint16_t host_f16(float f) {   // round to nearest even
    const _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
float host_f16_to_f32(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}
// the same finite garbage as an fp16 value (the residual stream's padding rows)
uint16_t poison_f16(size_t i, uint32_t seed) { return host_f16(host_bf16_to_f32(poison_bf16(i, seed))); }

constexpr size_t DBG_GUARD = 4096;          // bytes of sentinel on either side of every destination of the GEMM hooks
constexpr int DBG_SENTINEL = 0xA5;          // bf16 0xA5A5 = -7.17e-16, fp16 0xA5A5 = -0.02204, fp32 0xA5A5A5A5 = -2.87e-16: all finite
constexpr size_t DBG_GEMM_MAX = (size_t)1 << 26;   // elements of any one operand or destination

// A destination of the GEMM and row hooks: `bytes` of payload between two guard bands, all of it filled with the sentinel byte.
struct GuardedBuf {
    DevBuf buf;
    size_t bytes = 0;
    int make(size_t n) {
        bytes = round_up(n, 256);
        if (buf.ensure(bytes + 2 * DBG_GUARD)) return -1;
        MSE_HIP_TRY(hipMemset(buf.p, DBG_SENTINEL, bytes + 2 * DBG_GUARD));
        return 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(reinterpret_cast<char*>(buf.p) + DBG_GUARD); }
    int check(const char* what) const {   // the guard bands still hold the sentinel
        std::vector<uint8_t> g(2 * DBG_GUARD);
        MSE_HIP_TRY(hipMemcpy(g.data(), buf.p, DBG_GUARD, hipMemcpyDeviceToHost));
        MSE_HIP_TRY(hipMemcpy(g.data() + DBG_GUARD, reinterpret_cast<char*>(buf.p) + DBG_GUARD + bytes, DBG_GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < g.size(); i++)
            if (g[i] != DBG_SENTINEL)
                return fail(std::string("debug siglip: a launch wrote ") + (i < DBG_GUARD ? "before" : "past") + " its destination (" + what + ")");
        return 0;
    }
    template <typename T, typename F> int read(size_t n, float* out, F widen) const {
        std::vector<T> h(n);
        MSE_HIP_TRY(hipMemcpy(h.data(), as<T>(), n * sizeof(T), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < n; e++) out[e] = widen(h[e]);
        return 0;
    }
};

// [rows_pad][K] 16-bit operand from host fp32 [rows][K]: rounded by `conv`; rows past `rows` zero, or finite garbage when `poison`
template <typename Conv, typename Poison>
int upload_rows16(DevBuf& d, const float* src, size_t rows, size_t rows_pad, size_t K, Conv conv, bool poison, Poison garbage) {
    std::vector<uint16_t> h(rows_pad * K, 0);
    for (size_t e = 0; e < rows * K; e++) h[e] = conv(src[e]);
    for (size_t e = rows * K; poison && e < rows_pad * K; e++) h[e] = garbage(e);
    if (d.ensure(h.size() * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(d.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    return 0;
}
int upload_f32(DevBuf& d, const float* src, size_t n) {
    if (d.ensure(n * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(d.p, src, n * 4, hipMemcpyHostToDevice));
    return 0;
}

// the streams of a hook call: the engines' kind (non-blocking), with the fork / join events of a side-stream remainder launch
struct DbgStreams {
    hipStream_t main = nullptr, side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int make(bool with_side) {
        MSE_HIP_TRY(hipStreamCreateWithFlags(&main, hipStreamNonBlocking));
        if (!with_side) return 0;
        MSE_HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        MSE_HIP_TRY(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
        MSE_HIP_TRY(hipEventCreateWithFlags(&join, hipEventDisableTiming));
        return 0;
    }
    ~DbgStreams() {
        if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
        if (main) { (void)hipStreamSynchronize(main); (void)hipStreamDestroy(main); }
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
    }
};

// attention operands of the QKV scatter for `n_seq` sequences, as the engines allocate them, each a guarded destination
struct DbgQkv {
    GuardedBuf q, k, vt;
    size_t nq = 0, nk = 0, nvt = 0;
    int make(size_t n_seq, int heads, int n_pad, hipStream_t st) {
        const size_t mats = n_seq * heads;
        nq = mats * n_pad * DBG_DH_PAD; nk = mats * n_pad * attention_k_stride(); nvt = mats * DBG_DV_PAD * n_pad;
        if (q.make(nq * 2) || k.make(nk * 2) || vt.make(nvt * 2)) return -1;
        MSE_HIP_TRY(hipDeviceSynchronize());
        return launch_vt_ones_row(vt.as<uint16_t>(), mats, DBG_DH, DBG_DV_PAD, n_pad, st);
    }
    void attach(GemmLaunch& g, int heads, int n_pad) const {
        g.tokens = n_pad; g.q = q.as<uint16_t>(); g.k = k.as<uint16_t>(); g.vt = vt.as<uint16_t>(); g.heads = heads; g.dh = DBG_DH;
        g.dh_pad = DBG_DH_PAD; g.n_pad = n_pad; g.dv_pad = DBG_DV_PAD; g.kdh_pad = attention_k_stride();
    }
    int read(float* oq, float* ok, float* ovt) const {
        if (q.check("q") || k.check("k") || vt.check("vt")) return -1;
        return q.read<uint16_t>(nq, oq, host_bf16_to_f32) || k.read<uint16_t>(nk, ok, host_bf16_to_f32) || vt.read<uint16_t>(nvt, ovt, host_bf16_to_f32);
    }
};
// the towers' QKV geometry (launch_vt_ones_row and the scatter epilogues: 8-token / 8-column pieces inside q / k / v tiles)
bool dbg_qkv_ok(int rows, int N, int heads, int dh, int tokens) {
    return heads > 0 && dh == DBG_DH && tokens > 0 && tokens <= 8192 && N == 3 * heads * dh && (heads * dh) % 128 == 0 &&
           round_up((size_t)tokens, 32) >= 64 && rows % 8 == 0;
}
}  // namespace

extern "C" {

// Test hook for the towers' plain GEMM launches (mse.h: mse_debug_siglip_gemm_args).  x [rows][K], w [N][K] are host fp32, rounded here
// to bf16 (nearest even); bias, resid and pos stay fp32.  The operands are laid out as the towers lay them out (M = rows rounded up to
// 256 rows of x, every leading dimension = N) and ONE launch_gemm call is made with m_valid = rows, exactly as run_blocks and
// mse_siglip_encode_image fill in GemmLaunch: the kernel is therefore whichever launch_gemm_t picks for (epi, rows, N, K, skinny).
// Every destination is allocated between two guard bands and filled, guard bands included, with bytes 0xA5 before the launch; the
// hook fails if a guard byte changed, and returns the destinations WHOLE (padding included), widened to fp32, so that a test sees
// what a launch left of the sentinel.  A call with every output pointer NULL launches nothing and only fills in the derived sizes.
// Geometries the launchers (or the engines' buffers) do not accept are refused before anything is allocated.
//
// What a launch may do to padding, read from siglip_kernels.hip (rows = m_valid, M = rows rounded up to 256):
//   BF16 / GELU   skinny, 64 x 64 and 128 x 128 kernels (store_quad, !mok): rows rows .. rows rounded up to the tile height (64, 64,
//                 128) are ZEROED, rows above keep what they held.  First-generation and non-persistent ping-pong kernels (K < 256,
//                 or the GELU remainder): rows rows .. M are ZEROED.  Persistent kernel (K >= 256; its 128-column BF16 remainder
//                 too): stores are unconditional -- rows rows .. M are OVERWRITTEN with bias + x_pad . w, finite when x's padding
//                 rows are finite.  In every case: rows rows .. M hold zeros, finite values or what they held; nothing above M.
//   RESID / PATCH every kernel skips rows >= rows (mok / m < m_valid): the padding rows keep what they held.
//   QKV           a row m goes to sequence m / n_pad, token m % n_pad.  store_quad and the non-persistent kernels skip rows >= rows.
//                 The persistent kernels (K >= 256) scatter EVERY row below M: the entries of rows rows .. M (tokens of the last
//                 sequence past rows, and of up to (M - rows) / n_pad + 1 sequences behind it -- the engines allocate that slack)
//                 are OVERWRITTEN with finite values.  Columns dh .. of a q / K row, Vt's row-sum row dh and the rows above it are
//                 never written.  Tokens `tokens` .. n_pad of a sequence are rows below m_valid like any other.
//   PART          every slab is written up to rows rounded up to the tile height (64; 128 above SPLIT_T128_ROWS rows) with the raw
//                 sums of x's padding rows (finite); slab rows above that keep what they held.
// flags: 1 = x's padding rows hold finite garbage (poison_bf16, magnitude <= 1e4) instead of zeros; 2 = rows n_valid .. N of w hold the
// same garbage (columns < n_valid must not change); 4 = the 128-column remainder launch runs on a side stream between fork / join
// events of the engines' kind.
int mse_debug_siglip_gemm(mse_debug_siglip_gemm_args* p) {
    if (!p) return fail("debug siglip gemm: null argument");
    const int rows = p->rows, N = p->N, K = p->K, epi = p->epi;
    const bool qkv = epi == GEMM_EPI_QKV, part = epi == GEMM_EPI_PART;
    if (rows <= 0 || N <= 0 || K <= 0 || N % gemm_bn() || K % gemm_bk() || p->skinny < 0 || p->skinny > 4 || (p->gelu_tanh & ~1) || (p->flags & ~7))
        return fail("debug siglip gemm: rows, N, K > 0, N % 128 == 0, K % 64 == 0, skinny 0..4, gelu_tanh 0 / 1, flags 0..7");
    if (epi != GEMM_EPI_BF16 && epi != GEMM_EPI_GELU && epi != GEMM_EPI_RESID && epi != GEMM_EPI_PATCH && !qkv && !part)
        return fail("debug siglip gemm: epi must be BF16, GELU, RESID, PATCH, QKV or PART");
    const size_t M = round_up((size_t)rows, 256);
    if (M * K > DBG_GEMM_MAX || (size_t)N * K > DBG_GEMM_MAX || M * N > DBG_GEMM_MAX) return fail("debug siglip gemm: an operand exceeds 2^26 elements");
    const int n_valid = (p->flags & 2) ? p->n_valid : N;
    if (n_valid <= 0 || n_valid > N) return fail("debug siglip gemm: 0 < n_valid <= N");
    if (epi == GEMM_EPI_PATCH && (p->tokens <= 0 || (size_t)p->tokens * N > DBG_GEMM_MAX)) return fail("debug siglip gemm: PATCH needs tokens > 0");
    if (qkv && !dbg_qkv_ok(rows, N, p->heads, p->dh, p->tokens))
        return fail("debug siglip gemm: QKV needs dh == 72, heads % 16 == 0, N == 3 * heads * dh, 32 < tokens <= 8192, rows % 8 == 0");
    // K split: only what the towers ask for (gemm_small_ksplit: fc2 of one image; gemm_small_ksplit_short: the projection of one text)
    if (part && (p->ksplit < 2 || (p->ksplit != gemm_small_ksplit(rows, N, K) && p->ksplit != gemm_small_ksplit_short(rows, N, K))))
        return fail("debug siglip gemm: PART needs the ksplit that gemm_small_ksplit / gemm_small_ksplit_short give for (rows, N, K)");
    const int n_pad = qkv ? (int)round_up((size_t)p->tokens, 32) : 0;
    const size_t n_seq = qkv ? (M + n_pad - 1) / n_pad : 0;   // every row below M has a place: the persistent kernels scatter them all
    const size_t slab_rows = part ? (size_t)gemm_small_ksplit_rows(rows) : 0;
    if (qkv && n_seq * p->heads * n_pad * attention_k_stride() > DBG_GEMM_MAX) return fail("debug siglip gemm: an operand exceeds 2^26 elements");
    p->M = (int)M; p->n_pad = n_pad; p->n_seq = (int)n_seq; p->dh_pad = DBG_DH_PAD; p->kdh_pad = attention_k_stride(); p->dv_pad = DBG_DV_PAD;
    p->slab_rows = (int)slab_rows; p->cu_count = 0;
    if (!p->out && !p->q && !p->k && !p->vt) return 0;   // sizes only
    if (!p->x || !p->w || !p->bias || (qkv ? (!p->q || !p->k || !p->vt) : !p->out) || (epi == GEMM_EPI_RESID && !p->resid) ||
        (epi == GEMM_EPI_PATCH && !p->pos))
        return fail("debug siglip gemm: null argument");
    p->cu_count = device_cu_count();

    DevBuf dx, dw, dbias, dpos;
    if (upload_rows16(dx, p->x, rows, M, K, host_bf16, p->flags & 1, [](size_t e) { return poison_bf16(e, 0x58u); }) ||
        upload_rows16(dw, p->w, n_valid, N, K, host_bf16, p->flags & 2, [](size_t e) { return poison_bf16(e, 0x57u); }) ||
        upload_f32(dbias, p->bias, N))
        return -1;
    GuardedBuf out;
    DbgQkv o3;
    DbgStreams s;   // declared after every buffer: the streams are synchronised and destroyed before a buffer is freed
    if (s.make(p->flags & 4)) return -1;
    GemmLaunch g;
    g.x = dx.as<uint16_t>(); g.w = dw.as<uint16_t>(); g.bias = dbias.as<float>(); g.M = (int)M; g.N = N; g.K = K; g.m_valid = rows;
    g.skinny = p->skinny; g.gelu_tanh = p->gelu_tanh; g.side = s.side; g.ev_fork = s.fork; g.ev_join = s.join;
    const size_t out_elems = part ? (size_t)p->ksplit * slab_rows * N : M * N;
    if (qkv) {
        if (o3.make(n_seq, p->heads, n_pad, s.main)) return -1;
        o3.attach(g, p->heads, n_pad);
    } else if (epi == GEMM_EPI_RESID) {
        if (out.make(out_elems * 4)) return -1;
        MSE_HIP_TRY(hipMemcpy(out.as<float>(), p->resid, (size_t)rows * N * 4, hipMemcpyHostToDevice));
        g.resid = out.as<float>(); g.ldr = N;
    } else if (epi == GEMM_EPI_PATCH) {
        if (out.make(out_elems * 2) || upload_f32(dpos, p->pos, (size_t)p->tokens * N)) return -1;
        g.out_bf16 = out.as<uint16_t>(); g.ldo = N; g.ldr = N; g.pos = dpos.as<float>(); g.tokens = p->tokens;
    } else if (part) {
        if (out.make(out_elems * 4)) return -1;
        g.kpart = out.as<float>(); g.kpart_stride = slab_rows * N; g.ksplit = p->ksplit; g.ldr = N;
    } else {
        if (out.make(out_elems * 2)) return -1;
        g.out_bf16 = out.as<uint16_t>(); g.ldo = N;
    }
    MSE_HIP_TRY(hipDeviceSynchronize());   // uploads and fills ran on the null stream, which the hook's streams do not wait for
    if (launch_gemm(epi, g, s.main)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (qkv) return o3.read(p->q, p->k, p->vt);
    if (out.check("out")) return -1;
    if (epi == GEMM_EPI_RESID || part) return out.read<float>(out_elems, p->out, [](float v) { return v; });
    if (epi == GEMM_EPI_PATCH) return out.read<uint16_t>(out_elems, p->out, host_f16_to_f32);
    return out.read<uint16_t>(out_elems, p->out, host_bf16_to_f32);
}

// Test hook for the LayerNorm-fused launches of the image tower (mse.h: mse_debug_siglip_gemm_fused_args), with the same guarded,
// sentinel-filled destinations, whole-buffer outputs and size-only call as mse_debug_siglip_gemm.
//   consumers (epi QKV / GELU): x is the fp16 residual stream [rows][K] (host fp32, rounded here to fp16), w [N][K] bf16, gamma / beta
//     [K], bias [N]; launch_ln_fold, launch_row_stats over all M rows, launch_gemm_fused -- the order and arguments of
//     Encoder::fold_layernorms and run_blocks.  Returns the output and the (mean, 1/std) pairs [M][2].
//   producer (epi RESID_LN): x is the bf16 branch input [rows][K], w [N][K] with N = n_valid rounded up to 256, bias [N], xres the fp16
//     residual [rows][n_valid]; launch_gemm_fused with part_rows = M and a zeroed 4 KiB sink as Encoder::alloc_fused makes them, then
//     launch_ln_finalize.  Returns the updated residual [M][n_valid] and the (mean, 1/std) pairs [M][2].
// Padding (gemm8pp_kernel stores unconditionally): every row below M is computed and stored like a real one -- GELU output rows,
// the QKV entries of rows rows .. M (see mse_debug_siglip_gemm), residual rows and statistics rows rows .. M are OVERWRITTEN with
// finite values when the padding rows of the inputs are finite.  Columns n_valid .. N of the producer go to the sink: the residual has
// no such columns.  flags: 1 = the padding rows of x (and of xres) hold finite garbage instead of zeros; 2 = producer: rows n_valid .. N
// of w hold garbage.
int mse_debug_siglip_gemm_fused(mse_debug_siglip_gemm_fused_args* p) {
    if (!p) return fail("debug siglip gemm fused: null argument");
    const int rows = p->rows, N = p->N, K = p->K, epi = p->epi;
    const bool qkv = epi == GEMM_EPI_QKV, gelu = epi == GEMM_EPI_GELU, prod = epi == GEMM_EPI_RESID_LN;
    if (rows <= 0 || N <= 0 || K < 256 || N % 128 || K % 64 || (p->gelu_tanh & ~1) || (p->flags & ~3) || !(p->eps > 0.0f) || !(qkv || gelu || prod))
        return fail("debug siglip gemm fused: rows, N > 0, K >= 256, N % 128 == 0, K % 64 == 0, flags 0..3, eps > 0, epi QKV, GELU or RESID_LN");
    const size_t M = round_up((size_t)rows, 256);
    if (M * K > DBG_GEMM_MAX || (size_t)N * K > DBG_GEMM_MAX || M * N > DBG_GEMM_MAX) return fail("debug siglip gemm fused: an operand exceeds 2^26 elements");
    if (!prod && (K > 2048 || rows % 8)) return fail("debug siglip gemm fused: consumers need K <= 2048 (row statistics) and rows % 8 == 0");
    if (gelu && N % 256) return fail("debug siglip gemm fused: GELU needs N % 256 == 0");
    if (qkv && (!dbg_qkv_ok(rows, N, p->heads, p->dh, p->tokens) || p->heads * p->dh != K ||
                !gemm_fused_ok((int)M, K, 256, p->heads, p->dh, (int)round_up((size_t)p->tokens, 32), (int)round_up((size_t)p->tokens, 32), rows)))
        return fail("debug siglip gemm fused: QKV needs the towers' geometry (dh 72, heads % 16 == 0, K == heads * dh, N == 3 K, rows % 8 == 0)");
    const int n_valid = prod ? p->n_valid : N;
    if (prod && (n_valid <= 0 || n_valid % 64 || N != (int)round_up((size_t)n_valid, 256)))
        return fail("debug siglip gemm fused: RESID_LN needs n_valid % 64 == 0 and N == n_valid rounded up to 256");
    const int n_pad = qkv ? (int)round_up((size_t)p->tokens, 32) : 0;
    const size_t n_seq = qkv ? (M + n_pad - 1) / n_pad : 0;
    if (qkv && n_seq * p->heads * n_pad * attention_k_stride() > DBG_GEMM_MAX) return fail("debug siglip gemm fused: an operand exceeds 2^26 elements");
    p->M = (int)M; p->n_pad = n_pad; p->n_seq = (int)n_seq; p->dh_pad = DBG_DH_PAD; p->kdh_pad = attention_k_stride(); p->dv_pad = DBG_DV_PAD;
    if (!p->out && !p->q && !p->k && !p->vt && !p->stats) return 0;   // sizes only
    if (!p->x || !p->w || !p->bias || !p->stats || (qkv ? (!p->q || !p->k || !p->vt) : !p->out) || (prod ? !p->xres : (!p->gamma || !p->beta)))
        return fail("debug siglip gemm fused: null argument");

    DevBuf dx, dw, dbias, sink, dgamma, dbeta, w16, csum, bias2;
    GuardedBuf stats, xres, ln_part, out;
    DbgQkv o3;
    DbgStreams s;   // declared after every buffer: the streams are synchronised and destroyed before a buffer is freed
    if (s.make(false)) return -1;
    hipStream_t st = s.main;
    if (stats.make(M * 8)) return -1;
    GemmLaunch g;
    g.M = (int)M; g.N = N; g.K = K; g.m_valid = rows; g.gelu_tanh = p->gelu_tanh;
    if (upload_rows16(dw, p->w, n_valid, N, K, host_bf16, prod && (p->flags & 2), [](size_t e) { return poison_bf16(e, 0x57u); }) ||
        upload_f32(dbias, p->bias, N))
        return -1;
    if (prod) {
        if (upload_rows16(dx, p->x, rows, M, K, host_bf16, p->flags & 1, [](size_t e) { return poison_bf16(e, 0x58u); })) return -1;
        if (xres.make(M * n_valid * 2) || ln_part.make((size_t)(n_valid / 64) * M * 8) || sink.ensure(4096)) return -1;
        MSE_HIP_TRY(hipMemset(sink.p, 0, 4096));
        {
            std::vector<uint16_t> h(M * n_valid, 0);
            for (size_t e = 0; e < (size_t)rows * n_valid; e++) h[e] = host_f16(p->xres[e]);
            for (size_t e = (size_t)rows * n_valid; (p->flags & 1) && e < h.size(); e++) h[e] = poison_f16(e, 0x52u);
            MSE_HIP_TRY(hipMemcpy(xres.as<uint16_t>(), h.data(), h.size() * 2, hipMemcpyHostToDevice));
        }
        g.x = dx.as<uint16_t>(); g.w = dw.as<uint16_t>(); g.bias = dbias.as<float>();
        g.xres = xres.as<uint16_t>(); g.ldr = n_valid; g.part = ln_part.as<float>(); g.part_rows = M; g.n_valid = n_valid; g.sink = sink.p;
        MSE_HIP_TRY(hipDeviceSynchronize());
        if (launch_gemm_fused(GEMM_EPI_RESID_LN, g, st)) return -1;
        if (launch_ln_finalize(ln_part.as<float>(), M, n_valid / 64, M, p->eps, stats.as<float>(), st)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(st));
        if (xres.check("residual") || ln_part.check("statistics parts") || stats.check("statistics")) return -1;
        return xres.read<uint16_t>(M * n_valid, p->out, host_f16_to_f32) || stats.read<float>(M * 2, p->stats, [](float v) { return v; });
    }
    // consumers
    if (upload_rows16(dx, p->x, rows, M, K, host_f16, p->flags & 1, [](size_t e) { return poison_f16(e, 0x58u); })) return -1;
    if (upload_f32(dgamma, p->gamma, K) || upload_f32(dbeta, p->beta, K) || w16.ensure((size_t)N * K * 2) || csum.ensure((size_t)N * 4) ||
        bias2.ensure((size_t)N * 4))
        return -1;
    if (qkv) {
        if (o3.make(n_seq, p->heads, n_pad, st)) return -1;
        o3.attach(g, p->heads, n_pad);
    } else {
        if (out.make(M * N * 2)) return -1;
        g.out_bf16 = out.as<uint16_t>(); g.ldo = N;
    }
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (launch_ln_fold(dw.as<uint16_t>(), N, K, dgamma.as<float>(), dbeta.as<float>(), dbias.as<float>(), w16.as<uint16_t>(), csum.as<float>(),
                       bias2.as<float>(), st))
        return -1;
    if (launch_row_stats(dx.as<uint16_t>(), K, K, M, p->eps, stats.as<float>(), st)) return -1;
    g.x = dx.as<uint16_t>(); g.w = w16.as<uint16_t>(); g.bias = bias2.as<float>(); g.csum = csum.as<float>(); g.ln_stats = stats.as<float>();
    if (launch_gemm_fused(epi, g, st)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (stats.check("statistics") || stats.read<float>(M * 2, p->stats, [](float v) { return v; })) return -1;
    if (qkv) return o3.read(p->q, p->k, p->vt);
    if (out.check("out")) return -1;
    return out.read<uint16_t>(M * N, p->out, host_bf16_to_f32);
}

}  // extern "C"

namespace {
constexpr float DBG_ROWS_PAD = 1.0e4f;   // what the padding of the row hooks' OPERANDS holds: finite, exact in bf16 / fp16 / fp32, far from any input

// [rows][ld] operand from host fp32 [rows][width]: T(conv(v)); columns width .. ld hold DBG_ROWS_PAD
template <typename T, typename Conv>
int upload_ld(DevBuf& d, const float* src, size_t rows, size_t width, size_t ld, Conv conv) {
    std::vector<T> h(rows * ld, conv(DBG_ROWS_PAD));
    for (size_t r = 0; r < rows; r++)
        for (size_t c = 0; c < width; c++) h[r * ld + c] = conv(src[r * width + c]);
    if (d.ensure(h.size() * sizeof(T))) return -1;
    MSE_HIP_TRY(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
float same_f32(float v) { return v; }
bool dbg_rows_fit(size_t a, size_t b = 1, size_t c = 1) {   // a * b * c elements of one operand or destination
    return a && b && c && a <= DBG_GEMM_MAX && b <= DBG_GEMM_MAX && a * b <= DBG_GEMM_MAX && a * b * c <= DBG_GEMM_MAX;
}
}  // namespace

extern "C" {

// Test hooks for the towers' row kernels alone (mse.h: "row kernels"): each call makes ONE call of the launcher the towers use --
//   mse_debug_siglip_layernorm        launch_layernorm_d      layernorm_kernel / layernorm_wg_kernel (wg), x fp32 or fp16
//   mse_debug_siglip_patchify         launch_patchify         patchify8_kernel (P 14, k_pad % 8 == 0, k_pad <= 1024) or patchify_kernel
//   mse_debug_siglip_rgb8             launch_rgb8_to_nchw_f16
//   mse_debug_siglip_bmp24            launch_bmp24_to_nchw_f16
//   mse_debug_siglip_embed_tokens     launch_embed_tokens
//   mse_debug_siglip_f32_to_bf16_pad  launch_f32_to_bf16_pad
//   mse_debug_siglip_small_linear     launch_small_linear
//   mse_debug_siglip_l2norm           launch_l2norm
//   mse_debug_siglip_vt_ones_row      launch_vt_ones_row
// on a stream of the engines' kind, with the contract of the GEMM hooks.  Operands are host fp32 (u8 for the decoders, i64 for the
// tokens), compact ([rows][width]); the hook rounds them (nearest even) to the type the towers hold them in and lays them out with
// the leading dimension given, and the columns between the width and the leading dimension of an OPERAND hold 1e4, so a launch that
// read them shows.  Every DESTINATION -- LayerNorm's x included, which the kernel updates in place -- lies between two guard bands
// and is filled, guard bands included, with bytes 0xA5 before the launch (and, for x, before its rows are copied in); it comes back
// WHOLE, [rows][leading dimension], widened to fp32, so a test sees what the launch left of the sentinel; a changed guard byte fails
// the call.  A geometry the launcher refuses -- and a leading dimension smaller than its width or off the kernels' 4-element vector
// alignment, a null operand, more than 2^26 elements -- is refused before anything is allocated.
//
// What a launch writes, read from siglip_kernels.hip:
//   layernorm     x: with a delta (bf16 [rows][ldd], or n_parts fp32 slabs [part_rows][ldp] plus bias) columns 0 .. width of every
//                 row are rewritten with x + delta rounded to x's type; with NO delta x is not written at all.  out (bf16) / out_f32
//                 (either may be absent, both have rows of ldo): columns 0 .. width.  Columns width .. ld keep the sentinel.
//   patchify      every one of the B * tstride * k_pad elements: columns >= C P P and rows t >= tokens of an image are ZEROED
//                 (tokens = (H / P) * (W / P): pixels past the last whole patch are ignored, as by the stride-P convolution).
//   rgb8 / bmp24  every element of [B][C][H][W] fp16.       embed_tokens: every element of [rows][D] fp16.
//   f32_to_bf16_pad  every element of [rows_pad][cols_pad]; rows >= rows and columns >= cols are ZEROED.
//   small_linear  y[b][0 .. N]; columns N .. ldy keep the sentinel.     l2norm: every element of [B][width] of the outputs asked for.
//   vt_ones_row   row dh = 72 of each of the n_mats [80][n_pad] matrices = bf16 1.0; EVERYTHING else keeps the sentinel.
int mse_debug_siglip_layernorm(mse_debug_siglip_layernorm_args* p) {
    if (!p) return fail("debug siglip layernorm: null argument");
    const int rows = p->rows, width = p->width, ldx = p->ldx, ldo = p->ldo;
    if (rows <= 0 || width <= 0 || ldx < width || ldo < width || ldx % 4 || ldo % 4 || (p->x_is_f16 & ~1) || (p->wg & ~1) || !(p->eps > 0.0f))
        return fail("debug siglip layernorm: rows, width > 0, ldx, ldo >= width and multiples of 4, x_is_f16 0 / 1, wg 0 / 1, eps > 0");
    if (width % 4 || width > 2048) return fail("debug siglip layernorm: width must be a multiple of 4, at most 2048 (launch_layernorm_d)");
    if (p->parts && (p->delta || p->n_parts < 1 || !p->bias || p->ldp % 4))
        return fail("debug siglip layernorm: parts exclude a bf16 delta and need n_parts >= 1, a bias and ldp % 4 == 0 (launch_layernorm_d)");
    if (p->delta && (p->ldd < width || p->ldd % 4)) return fail("debug siglip layernorm: ldd >= width, a multiple of 4");
    if (p->parts && (p->ldp < width || p->part_rows < rows)) return fail("debug siglip layernorm: ldp >= width, part_rows >= rows");
    if (!dbg_rows_fit(rows, ldx) || !dbg_rows_fit(rows, ldo) || (p->delta && !dbg_rows_fit(rows, p->ldd)) ||
        (p->parts && !dbg_rows_fit(p->n_parts, p->part_rows, p->ldp)))
        return fail("debug siglip layernorm: an operand exceeds 2^26 elements");
    if (!p->x || !p->gamma || !p->beta || !p->x_out || (!p->out && !p->out_f32)) return fail("debug siglip layernorm: null argument");

    const size_t R = rows, W = width, xb = p->x_is_f16 ? 2 : 4;
    DevBuf ddelta, dparts, dbias, dgamma, dbeta;
    GuardedBuf x, out, out_f32;
    DbgStreams s;   // declared after every buffer: the stream is synchronised and destroyed before a buffer is freed
    if (s.make(false)) return -1;
    if (x.make(R * ldx * xb) || upload_f32(dgamma, p->gamma, W) || upload_f32(dbeta, p->beta, W)) return -1;
    if (p->x_is_f16) {
        std::vector<uint16_t> h(R * W);
        for (size_t e = 0; e < h.size(); e++) h[e] = host_f16(p->x[e]);
        MSE_HIP_TRY(hipMemcpy2D(x.as<char>(), (size_t)ldx * 2, h.data(), W * 2, W * 2, R, hipMemcpyHostToDevice));
    } else {
        MSE_HIP_TRY(hipMemcpy2D(x.as<char>(), (size_t)ldx * 4, p->x, W * 4, W * 4, R, hipMemcpyHostToDevice));
    }
    LnDelta d;
    if (p->delta) {
        if (upload_ld<uint16_t>(ddelta, p->delta, R, W, p->ldd, host_bf16)) return -1;
        d.bf16 = ddelta.as<uint16_t>(); d.ldd = p->ldd;
    } else if (p->parts) {
        std::vector<float> h((size_t)p->n_parts * p->part_rows * p->ldp, DBG_ROWS_PAD);
        for (size_t q = 0; q < (size_t)p->n_parts; q++)
            for (size_t r = 0; r < R; r++)
                for (size_t c = 0; c < W; c++) h[(q * p->part_rows + r) * p->ldp + c] = p->parts[(q * R + r) * W + c];
        if (upload_f32(dparts, h.data(), h.size()) || upload_f32(dbias, p->bias, W)) return -1;
        d.parts = dparts.as<float>(); d.n_parts = p->n_parts; d.part_stride = (size_t)p->part_rows * p->ldp; d.ldp = p->ldp;
        d.bias = dbias.as<float>();
    }
    if ((p->out && out.make(R * ldo * 2)) || (p->out_f32 && out_f32.make(R * ldo * 4))) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());   // uploads and fills ran on the null stream, which the hook's stream does not wait for
    if (launch_layernorm_d(x.as<void>(), p->x_is_f16, ldx, d, dgamma.as<float>(), dbeta.as<float>(), p->eps, width, R,
                           p->out ? out.as<uint16_t>() : nullptr, ldo, p->out_f32 ? out_f32.as<float>() : nullptr, p->wg, s.main))
        return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if (x.check("layernorm x") || (p->out && out.check("layernorm out")) || (p->out_f32 && out_f32.check("layernorm out_f32"))) return -1;
    if (p->x_is_f16 ? x.read<uint16_t>(R * ldx, p->x_out, host_f16_to_f32) : x.read<float>(R * ldx, p->x_out, same_f32)) return -1;
    if (p->out && out.read<uint16_t>(R * ldo, p->out, host_bf16_to_f32)) return -1;
    if (p->out_f32 && out_f32.read<float>(R * ldo, p->out_f32, same_f32)) return -1;
    return 0;
}

// img: host fp32 [B][C][H][W], rounded to fp16 when is_f16 (the towers' decoded images), else used as it is.  out: [B * tstride][k_pad].
int mse_debug_siglip_patchify(const float* img, int is_f16, int B, int C, int H, int W, int P, int k_pad, int tstride, float* out) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0 || k_pad <= 0 || tstride <= 0 || (is_f16 & ~1))
        return fail("debug siglip patchify: B, C, H, W, P, k_pad, tstride > 0, is_f16 0 / 1");
    if (H < P || W < P || k_pad < C * P * P) return fail("debug siglip patchify: H >= P, W >= P, k_pad >= C * P * P (launch_patchify)");
    if (!dbg_rows_fit(B, (size_t)C * H, W) || !dbg_rows_fit(B, tstride, k_pad)) return fail("debug siglip patchify: an operand exceeds 2^26 elements");
    if (!img || !out) return fail("debug siglip patchify: null argument");
    const size_t n_in = (size_t)B * C * H * W, n_out = (size_t)B * tstride * k_pad;
    DevBuf dimg;
    GuardedBuf dout;
    DbgStreams s;
    if (s.make(false)) return -1;
    if (is_f16 ? upload_ld<uint16_t>(dimg, img, 1, n_in, n_in, host_f16) : upload_f32(dimg, img, n_in)) return -1;
    if (dout.make(n_out * 2)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (launch_patchify(dimg.p, is_f16, B, C, H, W, P, k_pad, tstride, dout.as<uint16_t>(), s.main)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if (dout.check("patches")) return -1;
    return dout.read<uint16_t>(n_out, out, host_bf16_to_f32);
}

namespace {
int dbg_decode(const uint8_t* in, size_t n_in, const uint8_t* flags, size_t img_stride, int row_stride, int B, int C, int H, int W, float* out) {
    const size_t n_out = (size_t)B * C * H * W;
    DevBuf din, dflags;
    GuardedBuf dout;
    DbgStreams s;
    if (s.make(false)) return -1;
    if (din.ensure(n_in) || dout.make(n_out * 2) || (flags && dflags.ensure(B))) return -1;
    MSE_HIP_TRY(hipMemcpy(din.p, in, n_in, hipMemcpyHostToDevice));
    if (flags) MSE_HIP_TRY(hipMemcpy(dflags.p, flags, B, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (flags ? launch_bmp24_to_nchw_f16(din.as<uint8_t>(), img_stride, row_stride, dflags.as<uint8_t>(), dout.as<void>(), B, H, W, s.main)
              : launch_rgb8_to_nchw_f16(din.as<uint8_t>(), dout.as<void>(), B, C, H, W, s.main))
        return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if (dout.check("decoded image")) return -1;
    return dout.read<uint16_t>(n_out, out, host_f16_to_f32);
}
}  // namespace

// in: u8 [B][H][W][C] (RGB when C = 3).  out: fp16 [B][C][H][W].
int mse_debug_siglip_rgb8(const uint8_t* in, int B, int C, int H, int W, float* out) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !dbg_rows_fit(B, (size_t)C * H, W)) return fail("debug siglip rgb8: B, C, H, W > 0, at most 2^26 elements");
    if (!in || !out) return fail("debug siglip rgb8: null argument");
    return dbg_decode(in, (size_t)B * C * H * W, nullptr, 0, 0, B, C, H, W, out);
}

// in: B pixel arrays of 24-bit BMPs, img_stride bytes apart, rows of row_stride bytes, blue-green-red; flags[b] bit 0 = bottom row first.
int mse_debug_siglip_bmp24(const uint8_t* in, size_t img_stride, int row_stride, const uint8_t* flags, int B, int H, int W, float* out) {
    if (B <= 0 || H <= 0 || W <= 0 || !dbg_rows_fit(B, (size_t)3 * H, W) || row_stride < 3 * W || img_stride < (size_t)H * row_stride ||
        !dbg_rows_fit(B, img_stride))
        return fail("debug siglip bmp24: B, H, W > 0, row_stride >= 3 W, img_stride >= H * row_stride, at most 2^26 elements");
    if (!in || !flags || !out) return fail("debug siglip bmp24: null argument");
    return dbg_decode(in, (size_t)B * img_stride, flags, img_stride, row_stride, B, 3, H, W, out);
}

// tokens: i64 [rows]; tok_emb fp32 [vocab][D]; pos fp32 [ctx][D] (both stay fp32).  out: the fp16 residual rows [rows][D].
int mse_debug_siglip_embed_tokens(const int64_t* tokens, const float* tok_emb, const float* pos, int vocab, int ctx, int D, int rows, float* out) {
    if (vocab <= 0 || ctx <= 0 || D <= 0 || rows <= 0 || !dbg_rows_fit(vocab, D) || !dbg_rows_fit(ctx, D) || !dbg_rows_fit(rows, D))
        return fail("debug siglip embed tokens: vocab, ctx, D, rows > 0, at most 2^26 elements");
    if (D % 4) return fail("debug siglip embed tokens: D must be a multiple of 4 (launch_embed_tokens)");
    if (!tokens || !tok_emb || !pos || !out) return fail("debug siglip embed tokens: null argument");
    DevBuf dtok, demb, dpos;
    GuardedBuf dout;
    DbgStreams s;
    if (s.make(false)) return -1;
    if (dtok.ensure((size_t)rows * 8) || upload_f32(demb, tok_emb, (size_t)vocab * D) || upload_f32(dpos, pos, (size_t)ctx * D) ||
        dout.make((size_t)rows * D * 2))
        return -1;
    MSE_HIP_TRY(hipMemcpy(dtok.p, tokens, (size_t)rows * 8, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (launch_embed_tokens(dtok.as<int64_t>(), demb.as<float>(), dpos.as<float>(), vocab, ctx, D, rows, dout.as<uint16_t>(), s.main)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if (dout.check("embedded tokens")) return -1;
    return dout.read<uint16_t>((size_t)rows * D, out, host_f16_to_f32);
}

// in: host fp32 [rows][cols], laid out with rows of ld_in.  out: bf16 [rows_pad][cols_pad].
int mse_debug_siglip_f32_to_bf16_pad(const float* in, int rows, int cols, int ld_in, int rows_pad, int cols_pad, float* out) {
    if (rows <= 0 || cols <= 0 || ld_in < cols || rows_pad < rows || cols_pad < cols || !dbg_rows_fit(rows, ld_in) || !dbg_rows_fit(rows_pad, cols_pad))
        return fail("debug siglip f32 to bf16: rows, cols > 0, ld_in >= cols, rows_pad >= rows, cols_pad >= cols, at most 2^26 elements");
    if (!in || !out) return fail("debug siglip f32 to bf16: null argument");
    DevBuf din;
    GuardedBuf dout;
    DbgStreams s;
    if (s.make(false)) return -1;
    if (upload_ld<float>(din, in, rows, cols, ld_in, same_f32) || dout.make((size_t)rows_pad * cols_pad * 2)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (launch_f32_to_bf16_pad(din.as<float>(), rows, cols, ld_in, dout.as<uint16_t>(), rows_pad, cols_pad, s.main)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if (dout.check("padded bf16 rows")) return -1;
    return dout.read<uint16_t>((size_t)rows_pad * cols_pad, out, host_bf16_to_f32);
}

// x: host fp32 [B][K] (stays fp32, rows of ldx); w: host fp32 [N][K], rounded to bf16, rows of ldw; bias fp32 [N].  y: fp32 [B][ldy].
int mse_debug_siglip_small_linear(const float* x, int ldx, const float* w, int ldw, const float* bias, int K, int N, int B, int ldy, float* y) {
    if (K <= 0 || N <= 0 || B <= 0 || ldx < K || ldw < K || ldy < N || !dbg_rows_fit(B, ldx) || !dbg_rows_fit(N, ldw) || !dbg_rows_fit(B, ldy))
        return fail("debug siglip small linear: K, N, B > 0, ldx, ldw >= K, ldy >= N, at most 2^26 elements");
    if (!x || !w || !bias || !y) return fail("debug siglip small linear: null argument");
    DevBuf dx, dw, dbias;
    GuardedBuf dy;
    DbgStreams s;
    if (s.make(false)) return -1;
    if (upload_ld<float>(dx, x, B, K, ldx, same_f32) || upload_ld<uint16_t>(dw, w, N, K, ldw, host_bf16) || upload_f32(dbias, bias, N) ||
        dy.make((size_t)B * ldy * 4))
        return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (launch_small_linear(dx.as<float>(), ldx, dw.as<uint16_t>(), ldw, dbias.as<float>(), K, N, B, dy.as<float>(), ldy, s.main)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if (dy.check("small linear y")) return -1;
    return dy.read<float>((size_t)B * ldy, y, same_f32);
}

// x: host fp32 [B][width], rows of ldx.  out_f32 / out_f16 (either may be NULL): [B][width].
int mse_debug_siglip_l2norm(const float* x, int ldx, int width, int B, int normalize, float* out_f32, float* out_f16) {
    if (width <= 0 || B <= 0 || ldx < width || (normalize & ~1) || !dbg_rows_fit(B, ldx))
        return fail("debug siglip l2norm: width, B > 0, ldx >= width, normalize 0 / 1, at most 2^26 elements");
    if (!x || (!out_f32 && !out_f16)) return fail("debug siglip l2norm: null argument");
    const size_t n = (size_t)B * width;
    DevBuf dx;
    GuardedBuf d32, d16;
    DbgStreams s;
    if (s.make(false)) return -1;
    if (upload_ld<float>(dx, x, B, width, ldx, same_f32) || (out_f32 && d32.make(n * 4)) || (out_f16 && d16.make(n * 2))) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (launch_l2norm(dx.as<float>(), ldx, width, B, normalize, out_f32 ? d32.as<float>() : nullptr, out_f16 ? d16.as<uint16_t>() : nullptr, s.main))
        return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if ((out_f32 && (d32.check("l2norm fp32") || d32.read<float>(n, out_f32, same_f32))) ||
        (out_f16 && (d16.check("l2norm fp16") || d16.read<uint16_t>(n, out_f16, host_f16_to_f32))))
        return -1;
    return 0;
}

// out: the n_mats sentinel-filled bf16 [dv_pad][n_pad] matrices after the launch.
int mse_debug_siglip_vt_ones_row(int n_mats, int dh, int dv_pad, int n_pad, float* out) {
    if (n_mats <= 0 || n_pad <= 0 || dv_pad <= 0 || !dbg_rows_fit(n_mats, dv_pad, n_pad)) return fail("debug siglip vt ones row: n_mats, dv_pad, n_pad > 0, at most 2^26 elements");
    if (dh != DBG_DH || dv_pad != DBG_DV_PAD) return fail("debug siglip vt ones row: the row-sum row assumes dh 72, dv_pad 80 (launch_vt_ones_row)");
    if (!out) return fail("debug siglip vt ones row: null argument");
    const size_t n = (size_t)n_mats * dv_pad * n_pad;
    GuardedBuf vt;
    DbgStreams s;
    if (s.make(false)) return -1;
    if (vt.make(n * 2)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    if (launch_vt_ones_row(vt.as<uint16_t>(), n_mats, dh, dv_pad, n_pad, s.main)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s.main));
    if (vt.check("vt")) return -1;
    return vt.read<uint16_t>(n, out, host_bf16_to_f32);
}

// test hook: the residual stream ([batch*tokens][emb] fp32) as left by the last forward (after the last block)
int mse_siglip_debug_residual(mse_siglip* m, float* out) {
    if (!m || !m->last_batch) return fail("siglip: no forward has run");
    std::vector<uint16_t> h16((size_t)m->last_batch * m->tokens * m->D);
    MSE_HIP_TRY(hipMemcpy2D(h16.data(), (size_t)m->tokens * m->D * 2, m->x, (size_t)m->n_pad * m->D * 2, (size_t)m->tokens * m->D * 2,
                            m->last_batch, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < h16.size(); e++) {   // fp16 -> fp32 (exact)
        _Float16 hv;
        memcpy(&hv, &h16[e], 2);
        out[e] = (float)hv;
    }
    return 0;
}

}  // extern "C"
