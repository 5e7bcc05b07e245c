// Device resize in front of the image tower: `resize_for_embed_sync` (src/common.rs:31-54), i.e. a two-pass 8-bit convolution resize
// (Hamming when both sides shrink, Lanczos3 otherwise) of decoded RGB8 images or 24-bit BMP pixel arrays of any size.
// resize.hip: the host-side coefficient tables, the two kernels, the batch driver.  resize_api.hip: the C ABI.  DESIGN.md 3.25.
#pragma once
#include "common.h"
#include "runtime.h"
#include <memory>
#include <mutex>
#include <vector>

struct mse_siglip;

namespace mse {
namespace resize {

constexpr int SIDE_LIMIT = 16384;        // largest width / height of a source or a destination
constexpr int PRECISION_BITS = 22;       // fractional bits of an integer coefficient (32 - 8 - 2)
// Device staging of one sub-batch (sources, horizontal intermediates, staged u8 results, and the coefficient tables, which also
// exist once more on the host on their way up): a call is cut into sub-batches that stay below this, except that ONE image with its
// intermediate and its two tables always goes through, whatever it takes (16384 x 16384 -> 768 MiB + 18 MiB at 384).
constexpr size_t STAGE_BYTES = (size_t)256 << 20;
constexpr int SUB_BATCH_IMAGES = 1024;   // ... and of at most this many images

// coefficients of one axis, in -> out: for output i the taps bounds[2i] .. bounds[2i] + bounds[2i + 1] - 1 of the input with the
// integer weights coefs[i * ksize ..]; built on the host in double with libm (filter: MSE_RESIZE_HAMMING / MSE_RESIZE_LANCZOS3)
struct Table {
    int in = 0, out = 0, filter = 0, ksize = 0;
    std::vector<int32_t> bounds, coefs;
};
int table_ksize(int in, int out, int filter);
void build_table(int in, int out, int filter, Table& t);
// the AUTO rule (common.rs:44): one filter for both passes
int pick_filter(int w, int h, int out_w, int out_h, int filter);

// one source image in host memory: `bytes` bytes go up as they are; the top row starts at byte `row0` of them and the next row
// lies `stride` bytes further (negative: a bottom-up BMP); bgr: blue first
struct HostSrc {
    const uint8_t* data;
    size_t bytes, row0;
    long long stride;
    int w, h, bgr;
};

enum Epilogue { EPI_U8_HWC = 0, EPI_NCHW_F16 = 1 };

struct Context {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf src, mid, meta, out;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[4] = {0.0, 0.0, 0.0, 0.0};   // of the last call: upload, horizontal pass, vertical pass, whole call
    std::vector<unsigned char> meta_host;  // tables, descriptors and tile prefixes on their way up
    ~Context();
};
// stream: the stream the passes run on, or null for one of the context's own
std::shared_ptr<Context> make_context(hipStream_t stream);

// Resizes srcs[0 .. batch) to out_w x out_h.  EPI_U8_HWC: dst is HOST memory [batch][out_h][out_w][3]; EPI_NCHW_F16: dst is DEVICE
// memory [batch][3][out_h][out_w] fp16 holding x / 127.5 - 1.  Returns with the stream drained.  Arguments are the caller's to check.
int run(Context& c, const std::vector<HostSrc>& srcs, int out_w, int out_h, int filter, Epilogue epi, void* dst);

// the last call's times of any context, for mse_resize_timing
void last_timing(double ms[4]);

// the image engine as the resize sees it (siglip_api.hip)
struct TowerInput {
    std::recursive_mutex* call_mu;
    hipStream_t stream;
    void* img_dev;            // [max_batch][3][img_size][img_size] fp16: the forward pass's input buffer
    int img_size, in_chans, max_batch;
    bool finalized;
    std::shared_ptr<Context>* ctx;
};
TowerInput tower_input(mse_siglip* m);

}  // namespace resize
}  // namespace mse
