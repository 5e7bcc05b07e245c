// C ABI of the device resize (src/common.rs:31-54, `resize_for_embed_sync`): the coefficient tables alone, the resize alone, and
// the image tower's entry points for decoded images and BMP files of any size.  Every limit is checked before anything is launched.
#include "../../include/mse.h"
#include "resize.h"
#include <map>
#include <string>

using namespace mse;
using namespace mse::resize;

namespace {

int check_filter(int filter, bool allow_auto) {
    if (filter == MSE_RESIZE_HAMMING || filter == MSE_RESIZE_LANCZOS3 || (allow_auto && filter == MSE_RESIZE_AUTO)) return 0;
    return fail("resize: unknown filter " + std::to_string(filter));
}

int check_side(const char* what, long long v) {
    if (v >= 1 && v <= SIDE_LIMIT) return 0;
    return fail(std::string("resize: ") + what + " " + std::to_string(v) + " is outside 1 .. " + std::to_string(SIDE_LIMIT));
}

// decoded RGB8 images as sources; 0, or -1 with the error set
int rgb8_sources(const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, int batch, std::vector<HostSrc>& srcs) {
    if (!images || !widths || !heights) return fail("resize: null image, width or height list");
    srcs.resize(batch);
    for (int b = 0; b < batch; b++) {
        if (!images[b]) return fail("resize: image " + std::to_string(b) + " is null");
        if (check_side("width", widths[b]) || check_side("height", heights[b])) return -1;
        const size_t row = (size_t)widths[b] * 3;
        srcs[b] = HostSrc{images[b], row * heights[b], 0, (long long)row, (int)widths[b], (int)heights[b], 0};
    }
    return 0;
}

// the engine's context, made on its first _any call
Context* engine_context(const TowerInput& t) {
    if (!*t.ctx) *t.ctx = make_context(t.stream);
    return t.ctx->get();
}

int encode_any(mse_siglip* m, const TowerInput& t, const std::vector<HostSrc>& srcs, int filter, int normalize, float* out_f32, uint16_t* out_f16) {
    Context* c = engine_context(t);
    if (!c) return -1;
    if (run(*c, srcs, t.img_size, t.img_size, filter, EPI_NCHW_F16, t.img_dev)) return -1;
    return mse_siglip_encode_image(m, t.img_dev, 1, 1, (int)srcs.size(), normalize, out_f32, out_f16);
}

int check_engine_call(const TowerInput& t, int batch, int filter) {
    if (!t.finalized) return fail("siglip: call mse_siglip_finalize after loading the weights");
    if (batch <= 0 || batch > t.max_batch) return fail("siglip: batch exceeds max_batch");
    if (t.in_chans != 3) return fail("siglip: image input needs a 3-channel model");
    return check_filter(filter, true);
}

}  // namespace

extern "C" {

int mse_resize_coeffs(int in, int out, int filter, int* ksize, int32_t* bounds_out, int32_t* coefs_out) {
    if (check_side("input length", in) || check_side("output length", out) || check_filter(filter, false)) return -1;
    if (!ksize) return fail("resize: null ksize");
    *ksize = table_ksize(in, out, filter);
    if (!bounds_out && !coefs_out) return 0;
    Table t;
    build_table(in, out, filter, t);
    if (bounds_out) std::copy(t.bounds.begin(), t.bounds.end(), bounds_out);
    if (coefs_out) std::copy(t.coefs.begin(), t.coefs.end(), coefs_out);
    return 0;
}

int mse_resize_pick_filter(int w, int h, int out_w, int out_h, int filter) {
    if (check_side("width", w) || check_side("height", h) || check_side("output width", out_w) || check_side("output height", out_h) ||
        check_filter(filter, true)) return -1;
    return pick_filter(w, h, out_w, out_h, filter);
}

int mse_resize_rgb8(const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, int batch, int out_w, int out_h, int filter,
                    uint8_t* out_hwc_u8) {
    if (!out_hwc_u8) return fail("resize: null output");
    if (batch <= 0) return fail("resize: batch must be at least 1");
    if (check_side("output width", out_w) || check_side("output height", out_h) || check_filter(filter, true)) return -1;
    std::vector<HostSrc> srcs;
    if (rgb8_sources(images, widths, heights, batch, srcs)) return -1;
    // One context (stream, events, staging) PER DEVICE for the calls that bring no engine, on the caller's current device; one such
    // call at a time.  The map is never destroyed: at process exit the HIP runtime may be gone before a static's destructor runs,
    // and a destructor that synchronises, destroys a stream and frees device memory must not run then.
    static std::mutex mu;
    static auto* contexts = new std::map<int, std::shared_ptr<Context>>();
    std::lock_guard<std::mutex> lock(mu);
    int device = 0;
    MSE_HIP_TRY(hipGetDevice(&device));
    std::shared_ptr<Context>& ctx = (*contexts)[device];
    if (!ctx) ctx = make_context(nullptr);
    if (!ctx) return -1;
    return run(*ctx, srcs, out_w, out_h, filter, EPI_U8_HWC, out_hwc_u8);
}

int mse_siglip_encode_rgb8_any(mse_siglip* m, const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, int batch, int filter,
                               int normalize, float* out_f32, uint16_t* out_f16) {
    if (!m) return fail("null engine");
    const TowerInput t = tower_input(m);
    std::lock_guard<std::recursive_mutex> call_lock(*t.call_mu);
    if (check_engine_call(t, batch, filter)) return -1;
    std::vector<HostSrc> srcs;
    if (rgb8_sources(images, widths, heights, batch, srcs)) return -1;
    return encode_any(m, t, srcs, filter, normalize, out_f32, out_f16);
}

int mse_siglip_encode_bmp_any(mse_siglip* m, const uint8_t* const* bmps, const size_t* sizes, int batch, int filter, int normalize,
                              float* out_f32, uint16_t* out_f16) {
    if (!m) return fail("null engine");
    if (!bmps || !sizes) return fail("resize: null file or size list");
    const TowerInput t = tower_input(m);
    std::lock_guard<std::recursive_mutex> call_lock(*t.call_mu);
    if (check_engine_call(t, batch, filter)) return -1;
    std::vector<HostSrc> srcs(batch);
    for (int b = 0; b < batch; b++) {
        if (!bmps[b]) return fail("resize: file " + std::to_string(b) + " is null");
        uint32_t w = 0, h = 0, off = 0;
        int bu = 0;
        if (mse_bmp24_info(bmps[b], sizes[b], &w, &h, &off, &bu)) return -1;   // ... and the pixel array lies inside the file
        if (check_side("width", w) || check_side("height", h)) return -1;
        // rows of 3w bytes rounded up to 4, blue first, bottom row first unless the header's height was negative
        const size_t stride = ((size_t)w * 3 + 3) & ~(size_t)3;
        srcs[b] = HostSrc{bmps[b] + off, stride * h, bu ? stride * (h - 1) : 0, bu ? -(long long)stride : (long long)stride, (int)w, (int)h, 1};
    }
    return encode_any(m, t, srcs, filter, normalize, out_f32, out_f16);
}

int mse_debug_siglip_resize_nchw(mse_siglip* m, int batch, uint16_t* out) {
    if (!m || !out) return fail("debug resize: null argument");
    const TowerInput t = tower_input(m);
    std::lock_guard<std::recursive_mutex> call_lock(*t.call_mu);
    if (batch <= 0 || batch > t.max_batch) return fail("siglip: batch exceeds max_batch");
    MSE_HIP_TRY(hipMemcpyAsync(out, t.img_dev, (size_t)batch * 3 * t.img_size * t.img_size * 2, hipMemcpyDeviceToHost, t.stream));
    MSE_HIP_TRY(hipStreamSynchronize(t.stream));
    return 0;
}

int mse_resize_timing(double* ms) {
    if (!ms) return fail("resize timing: null argument");
    last_timing(ms);
    return 0;
}

}  // extern "C"
