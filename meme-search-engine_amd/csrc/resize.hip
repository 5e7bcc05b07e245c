// Two-pass 8-bit convolution resize on the device: what `resize_for_embed_sync` (src/common.rs:31-54) does to
// every image before it is embedded -- squash to exactly image_size, Hamming window when both sides shrink, Lanczos3 otherwise.
// The arithmetic is Pillow's 8-bit resample restated (tests/resize_ref.py): filter weights in double on the HOST (libm's sin / cos;
// the device's differ in the last bit and one flipped coefficient shows in the pixels), normalised per output, rounded to integers
// of 22 fractional bits; a pass is acc = 2^21 + sum coef * pixel in int32, output clamp(acc >> 22, 0, 255).  Integer sums are
// order-free, so the kernels add in whatever order suits them.  Horizontal pass first into a u8 intermediate, then vertical; a
// pass whose input and output lengths agree is skipped.
//
// One launch per pass for the whole (sub-)batch of mixed sizes: a device table of per-image descriptors and a prefix over the
// images' tile counts tell a workgroup which tile of which image it is.
#include "resize.h"
#include "../../include/mse.h"
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <tuple>

namespace mse {
namespace resize {

// ---- coefficient tables (host) ----------------------------------------------------------------------------------
namespace {
double hamming_filter(double x) {
    // the window's constants are float32 in Pillow (0.54f + 0.46f * cos(x) in double): with the double constants about two
    // outputs in 4e5 differ by one
    const double A = (double)0.54f, B = (double)0.46f;
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * M_PI;
    return sin(x) / x * (A + B * cos(x));
}
double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
double lanczos3_filter(double x) {
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}
double filter_support(int filter) { return filter == MSE_RESIZE_HAMMING ? 1.0 : 3.0; }
}  // namespace

int table_ksize(int in, int out, int filter) {
    double fs = (double)in / out;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(filter_support(filter) * fs) * 2 + 1;
}

void build_table(int in, int out, int filter, Table& t) {
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    t.in = in; t.out = out; t.filter = filter; t.ksize = ksize;
    t.bounds.assign((size_t)out * 2, 0);
    t.coefs.assign((size_t)out * ksize, 0);
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; x++) {
            const double a = (x + xmin - center + 0.5) * ss;
            w[x] = filter == MSE_RESIZE_HAMMING ? hamming_filter(a) : lanczos3_filter(a);
            ww += w[x];
        }
        int32_t* k = &t.coefs[(size_t)xx * ksize];
        for (int x = 0; x < n; x++) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (double)(1 << PRECISION_BITS));
        }
        t.bounds[(size_t)xx * 2] = xmin;
        t.bounds[(size_t)xx * 2 + 1] = n;
    }
}

int pick_filter(int w, int h, int out_w, int out_h, int filter) {
    if (filter != MSE_RESIZE_AUTO) return filter;
    return (w > out_w && h > out_h) ? MSE_RESIZE_HAMMING : MSE_RESIZE_LANCZOS3;
}

// ---- kernels ----------------------------------------------------------------------------------------------------
namespace {

// one image of a launch.  A table is addressed by its first word in the launch's pool of int32 words:
// [0] ksize, [1] outputs, then bounds [outputs][2] = (first tap, taps), then coefs [outputs][ksize]
struct ImgDesc {
    const uint8_t* src;     // first byte of the TOP row
    long long src_stride;   // bytes from a row to the one below it (negative: bottom-up BMP)
    uint8_t* mid;           // horizontal pass's output: [h] rows of mid_pitch bytes, RGB
    int w, h;
    int bgr;                // source channel order: 0 RGB, 1 BGR
    int mid_pitch;
    int tab_h, tab_v;       // table of each pass, or -1 when the pass is skipped (equal lengths)
};

// Horizontal pass: a tile is HT_ROWS rows x HT_OX output pixels of one image
constexpr int HT_OX = 32;             // output pixels of a tile
constexpr int HT_ROWS = 8;            // rows of a tile
constexpr int H_THREADS = HT_OX * HT_ROWS;
constexpr int H_SEG_BYTES = 40960;    // most LDS for a tile's source row segments (each staged once, shared by the tile's outputs)
constexpr int H_COEF_WORDS = 4096;    // most LDS for a tile's slice of the coefficient table (16 KiB: 32 outputs of up to 128 taps)
// Vertical pass: a tile is VT_OY output rows x V_THREADS * V_BYTES bytes of them
constexpr int VT_OY = 8;              // output rows of a tile
constexpr int V_THREADS = 64;          // one wave: the tower's 1152-byte rows are 4.5 tiles wide (a 1024-byte tile would leave 7/8 of a second workgroup idle)
constexpr int V_BYTES = 4;            // consecutive bytes of a row per thread
constexpr int VT_XBYTES = V_THREADS * V_BYTES;

__device__ __forceinline__ int find_image(const unsigned* __restrict__ prefix, int batch, unsigned tile) {
    int lo = 0, hi = batch;             // prefix[lo] <= tile < prefix[hi]
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (prefix[m] <= tile) lo = m; else hi = m;
    }
    return lo;
}

template <typename KP, typename PP>
__device__ __forceinline__ void h_accumulate(KP k, PP p, int n, int& a0, int& a1, int& a2) {
    for (int x = 0; x < n; x++) {
        const int c = k[x];
        a0 += c * (int)p[3 * x]; a1 += c * (int)p[3 * x + 1]; a2 += c * (int)p[3 * x + 2];
    }
}

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> PRECISION_BITS;     // arithmetic shift
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The pass that streams the big image.  The source bytes a tile needs of each of its rows -- from the first tap of its first output
// to the last tap of its last -- are staged in LDS once with 16-byte global loads and shared by the tile's outputs; 3 * w is rarely
// a multiple of 16, so a row's segment starts at any byte: the loads start at the 16-byte boundary below it and the segment keeps
// its misalignment in LDS.  (The source buffer is padded so that those whole 16-byte pieces lie inside it: run_sub.)  The tile's slice
// of the coefficient table is staged too.  A tile whose segments or coefficients do not fit (a shrink by hundreds) reads them through L2.
// The launch brings as much dynamic LDS as its largest tile that fits needs (seg_cap bytes of segments, a multiple of 16, then coef_cap
// words), at most H_SEG_BYTES + 4 * H_COEF_WORDS: 3 KiB for 1024 -> 384, so that the CU holds as many workgroups as it has wave slots for.
__global__ __launch_bounds__(H_THREADS) void resize_h_kernel(const ImgDesc* __restrict__ descs, const unsigned* __restrict__ prefix, int batch,
                                                             const int32_t* __restrict__ pool, int out_w, int seg_cap, int coef_cap) {
    extern __shared__ __align__(16) uint8_t h_lds[];
    uint8_t* seg = h_lds;
    int32_t* kc = reinterpret_cast<int32_t*>(h_lds + seg_cap);
    const int tid = threadIdx.x;
    const int img = find_image(prefix, batch, blockIdx.x);
    const ImgDesc d = descs[img];
    const int local = (int)(blockIdx.x - prefix[img]);
    const int tiles_x = (out_w + HT_OX - 1) / HT_OX;
    const int ox0 = (local % tiles_x) * HT_OX, y0 = (local / tiles_x) * HT_ROWS;
    const int nox = min(HT_OX, out_w - ox0), nrows = min(HT_ROWS, d.h - y0);
    const int32_t* tab = pool + d.tab_h;
    const int ksize = tab[0];
    const int32_t* bounds = tab + 2;
    const int32_t* coefs = tab + 2 + 2 * (size_t)out_w;
    const int xb = bounds[2 * ox0];
    const int xe = bounds[2 * (ox0 + nox - 1)] + bounds[2 * (ox0 + nox - 1) + 1];   // first taps and tap ends both never decrease
    const int seg_bytes = (xe - xb) * 3;
    const int pitch = (seg_bytes + 15 + 15) & ~15;    // a row in LDS: up to 15 bytes of misalignment, the segment, rounded to 16
    const bool stage_px = (long long)pitch * nrows <= seg_cap;
    const bool stage_k = nox * ksize <= coef_cap;
    if (stage_k)
        for (int i = tid; i < nox * ksize; i += H_THREADS) kc[i] = coefs[(size_t)ox0 * ksize + i];
    if (stage_px) {
        const int cpr = pitch >> 4;
        for (int i = tid; i < nrows * cpr; i += H_THREADS) {
            const int r = i / cpr, c = i % cpr;
            const uint8_t* a = d.src + (long long)(y0 + r) * d.src_stride + (long long)xb * 3;
            const int mis = (int)((uintptr_t)a & 15);
            if (c * 16 < mis + seg_bytes)
                *reinterpret_cast<uint4*>(seg + r * pitch + c * 16) = *reinterpret_cast<const uint4*>(a - mis + c * 16);
        }
    }
    __syncthreads();
    const int r = tid / HT_OX, lx = tid % HT_OX;
    if (r >= nrows || lx >= nox) return;
    const int xmin = bounds[2 * (ox0 + lx)], n = bounds[2 * (ox0 + lx) + 1];
    const uint8_t* row = d.src + (long long)(y0 + r) * d.src_stride;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    if (stage_px) {
        const int mis = (int)((uintptr_t)(row + (long long)xb * 3) & 15);
        const uint8_t* p = seg + r * pitch + mis + (xmin - xb) * 3;
        if (stage_k) h_accumulate(kc + lx * ksize, p, n, a0, a1, a2);
        else h_accumulate(coefs + (size_t)(ox0 + lx) * ksize, p, n, a0, a1, a2);
    } else {
        const uint8_t* p = row + (long long)xmin * 3;
        if (stage_k) h_accumulate(kc + lx * ksize, p, n, a0, a1, a2);
        else h_accumulate(coefs + (size_t)(ox0 + lx) * ksize, p, n, a0, a1, a2);
    }
    uint8_t* o = d.mid + (size_t)(y0 + r) * d.mid_pitch + (size_t)(ox0 + lx) * 3;
    o[0] = clip8(d.bgr ? a2 : a0); o[1] = clip8(a1); o[2] = clip8(d.bgr ? a0 : a2);
}

// Vertical pass and epilogue.  It reads the intermediate, or the source itself when the horizontal pass was skipped.  A thread owns
// V_BYTES consecutive bytes of VT_OY output rows and walks the input rows those outputs need ONCE, top to bottom: each input byte is
// loaded once per tile and added into whichever of the outputs have a tap on that row.  The taps and coefficients are the same for
// the whole workgroup (scalar loads through the constant cache), so no LDS is used here.  tab_v < 0: the rows are copied (the
// epilogue still runs).
// EPI_U8_HWC: dst [image][out_h][out_w][3] u8.  EPI_NCHW_F16: dst [image][3][out_h][out_w] fp16, x / 127.5 - 1 in fp32 and round to
// nearest even -- rgb8_to_nchw_f16_kernel's arithmetic (siglip_kernels.hip), bit for bit.
template <int EPI>
__global__ __launch_bounds__(V_THREADS) void resize_v_kernel(const ImgDesc* __restrict__ descs, const unsigned* __restrict__ prefix, int batch,
                                                             const int32_t* __restrict__ pool, int out_w, int out_h, void* __restrict__ dst) {
    const int img = find_image(prefix, batch, blockIdx.x);
    const ImgDesc d = descs[img];
    const int local = (int)(blockIdx.x - prefix[img]);
    const int row_bytes = out_w * 3;
    const int tiles_x = (row_bytes + VT_XBYTES - 1) / VT_XBYTES;
    const int j0 = (local % tiles_x) * VT_XBYTES + (int)threadIdx.x * V_BYTES;
    const int oy0 = (local / tiles_x) * VT_OY;
    const int noy = min(VT_OY, out_h - oy0);
    if (j0 >= row_bytes) return;
    const int nb = min(V_BYTES, row_bytes - j0);
    const bool from_mid = d.tab_h >= 0;
    const uint8_t* in = from_mid ? d.mid : d.src;
    const long long in_pitch = from_mid ? (long long)d.mid_pitch : d.src_stride;
    const bool bgr = !from_mid && d.bgr;
    int sj[V_BYTES];                       // source byte of each of the thread's bytes (BGR: the pixel's bytes mirrored)
#pragma unroll
    for (int b = 0; b < V_BYTES; b++) {
        const int j = j0 + b;
        sj[b] = bgr ? j - j % 3 + 2 - j % 3 : j;
    }
    const bool dword = !bgr && nb == V_BYTES && (((uintptr_t)in | (uintptr_t)in_pitch) & 3) == 0;   // j0 is a multiple of 4
    int acc[VT_OY][V_BYTES];
    if (d.tab_v < 0) {
#pragma unroll
        for (int o = 0; o < VT_OY; o++)
#pragma unroll
            for (int b = 0; b < V_BYTES; b++)
                acc[o][b] = (o < noy && b < nb) ? ((int)in[(long long)(oy0 + o) * in_pitch + sj[b]] << PRECISION_BITS) : 0;
    } else {
        const int32_t* tab = pool + d.tab_v;
        const int ksize = tab[0];
        const int32_t* bounds = tab + 2;
        const int32_t* coefs = tab + 2 + 2 * (size_t)out_h;
        int ymin[VT_OY], yn[VT_OY];
#pragma unroll
        for (int o = 0; o < VT_OY; o++) {
            ymin[o] = o < noy ? bounds[2 * (oy0 + o)] : 0;
            yn[o] = o < noy ? bounds[2 * (oy0 + o) + 1] : 0;
#pragma unroll
            for (int b = 0; b < V_BYTES; b++) acc[o][b] = 1 << (PRECISION_BITS - 1);
        }
        const int ya = ymin[0], yb = bounds[2 * (oy0 + noy - 1)] + bounds[2 * (oy0 + noy - 1) + 1];   // neither bound ever decreases
        for (int y = ya; y < yb; y++) {
            const uint8_t* rp = in + (long long)y * in_pitch;
            int px[V_BYTES];
            if (dword) {
                const unsigned v = *reinterpret_cast<const unsigned*>(rp + j0);
#pragma unroll
                for (int b = 0; b < V_BYTES; b++) px[b] = (int)((v >> (8 * b)) & 255u);
            } else {
#pragma unroll
                for (int b = 0; b < V_BYTES; b++) px[b] = b < nb ? (int)rp[sj[b]] : 0;
            }
#pragma unroll
            for (int o = 0; o < VT_OY; o++) {
                const int t = y - ymin[o];
                if ((unsigned)t < (unsigned)yn[o]) {
                    const int c = coefs[(size_t)(oy0 + o) * ksize + t];
#pragma unroll
                    for (int b = 0; b < V_BYTES; b++) acc[o][b] += c * px[b];
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < VT_OY; o++) {
        if (o >= noy) continue;
        const int oy = oy0 + o;
#pragma unroll
        for (int b = 0; b < V_BYTES; b++) {
            if (b >= nb) continue;
            const int j = j0 + b;
            const uint8_t v = clip8(acc[o][b]);
            if (EPI == EPI_U8_HWC) {
                reinterpret_cast<uint8_t*>(dst)[((size_t)img * out_h + oy) * row_bytes + j] = v;
            } else {
                const int x = j / 3, ch = j % 3;
                const float f = (float)v / 127.5f - 1.0f;
                reinterpret_cast<_Float16*>(dst)[(((size_t)img * 3 + ch) * out_h + oy) * out_w + x] = (_Float16)f;
            }
        }
    }
}

std::mutex g_timing_mu;
double g_timing[4] = {0.0, 0.0, 0.0, 0.0};

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

using TableKey = std::tuple<int, int, int>;   // (in, out, filter)

// words a table takes in the pool: ksize, outputs, bounds, coefficients
size_t table_words(int in, int out, int filter) { return 2 + (size_t)out * 2 + (size_t)out * table_ksize(in, out, filter); }

// device bytes image `s` adds to a sub-batch that already holds the tables `have`: its upload, its intermediate, its u8 result when
// that is staged too, and the coefficient tables it is the first to need (they are added to `have`)
size_t image_cost(const HostSrc& s, int out_w, int out_h, int filter, Epilogue epi, std::set<TableKey>& have) {
    size_t b = up16(s.bytes);
    if (s.w != out_w) b += up16((size_t)out_w * 3) * s.h;
    if (epi == EPI_U8_HWC) b += (size_t)out_w * out_h * 3;
    const int f = pick_filter(s.w, s.h, out_w, out_h, filter);
    if (s.w != out_w && have.insert(TableKey(s.w, out_w, f)).second) b += table_words(s.w, out_w, f) * 4;
    if (s.h != out_h && have.insert(TableKey(s.h, out_h, f)).second) b += table_words(s.h, out_h, f) * 4;
    return b;
}

// images [i0, i1) of the call: tables, descriptors, upload, the two launches, download of a u8 result
int run_sub(Context& c, const std::vector<HostSrc>& srcs, size_t i0, size_t i1, int out_w, int out_h, int filter, Epilogue epi, void* dst) {
    const int nb = (int)(i1 - i0);
    hipStream_t st = c.stream;
    // tables, deduplicated by (in, out, filter): where each starts in the pool, and of one that serves a horizontal pass the LDS
    // bytes one row segment of each of its tiles takes
    struct Entry { int at; Table t; std::vector<int> pitch; };
    std::vector<int32_t> pool;
    std::map<TableKey, Entry> tables;
    auto table = [&](int in, int out, int f) -> Entry& {
        auto it = tables.find(std::make_tuple(in, out, f));
        if (it != tables.end()) return it->second;
        Entry& e = tables[std::make_tuple(in, out, f)];
        build_table(in, out, f, e.t);
        e.at = (int)pool.size();
        pool.push_back(e.t.ksize); pool.push_back(out);
        pool.insert(pool.end(), e.t.bounds.begin(), e.t.bounds.end());
        pool.insert(pool.end(), e.t.coefs.begin(), e.t.coefs.end());
        return e;
    };
    // dynamic LDS of the horizontal launch: what its largest tile that fits within H_SEG_BYTES / H_COEF_WORDS needs (so a tile stages
    // exactly when it fits within those two constants, whatever the other images of the launch are)
    int seg_cap = 0, coef_cap = 0;
    auto h_lds_need = [&](Entry& e, int h) {
        const Table& t = e.t;
        if (e.pitch.empty())
            for (int ox0 = 0; ox0 < t.out; ox0 += HT_OX) {
                const int last = std::min(ox0 + HT_OX, t.out) - 1;
                e.pitch.push_back(((t.bounds[2 * last] + t.bounds[2 * last + 1] - t.bounds[2 * ox0]) * 3 + 30) & ~15);
            }
        for (size_t tile = 0; tile < e.pitch.size(); tile++) {
            const int nox = std::min(HT_OX, t.out - (int)tile * HT_OX);
            if (nox * t.ksize <= H_COEF_WORDS) coef_cap = std::max(coef_cap, nox * t.ksize);
            for (int rows : {std::min(HT_ROWS, h), h % HT_ROWS})      // a full band, and the last band of an image
                if (rows > 0 && (long long)e.pitch[tile] * rows <= H_SEG_BYTES) seg_cap = std::max(seg_cap, e.pitch[tile] * rows);
        }
    };
    std::vector<ImgDesc> descs(nb);
    std::vector<size_t> src_off(nb), mid_off(nb);
    std::vector<unsigned> pre_h(nb + 1, 0), pre_v(nb + 1, 0);
    size_t src_bytes = 0, mid_bytes = 0;
    const unsigned v_tiles = (unsigned)((out_h + VT_OY - 1) / VT_OY) * (unsigned)((out_w * 3 + VT_XBYTES - 1) / VT_XBYTES);
    for (int i = 0; i < nb; i++) {
        const HostSrc& s = srcs[i0 + i];
        const int f = pick_filter(s.w, s.h, out_w, out_h, filter);
        ImgDesc& d = descs[i];
        d.w = s.w; d.h = s.h; d.bgr = s.bgr; d.src_stride = s.stride;
        d.tab_h = d.tab_v = -1;
        if (s.w != out_w) {
            Entry& e = table(s.w, out_w, f);
            h_lds_need(e, s.h);
            d.tab_h = e.at;
        }
        if (s.h != out_h) d.tab_v = table(s.h, out_h, f).at;
        src_off[i] = src_bytes;
        src_bytes += up16(s.bytes);
        d.mid_pitch = (int)up16((size_t)out_w * 3);
        mid_off[i] = mid_bytes;
        if (d.tab_h >= 0) mid_bytes += (size_t)d.mid_pitch * s.h;
        const unsigned h_tiles = d.tab_h >= 0 ? (unsigned)((s.h + HT_ROWS - 1) / HT_ROWS) * (unsigned)((out_w + HT_OX - 1) / HT_OX) : 0u;
        if ((unsigned long long)pre_h[i] + h_tiles > 0x7fffffffull) return fail("resize: too many tiles in one sub-batch");
        pre_h[i + 1] = pre_h[i] + h_tiles;
        pre_v[i + 1] = pre_v[i] + v_tiles;
    }
    // 16 bytes past the last image: the horizontal pass loads whole 16-byte pieces around a row segment, and every image starts on
    // a 16-byte boundary of an allocation that is itself aligned, so those pieces lie inside [src, src + src_bytes + 16)
    const size_t out_img = (size_t)out_w * out_h * 3;
    if (c.src.ensure(src_bytes + 16) || c.mid.ensure(mid_bytes + 16)) return -1;
    if (epi == EPI_U8_HWC && c.out.ensure(out_img * nb)) return -1;
    for (int i = 0; i < nb; i++) {
        descs[i].src = c.src.as<uint8_t>() + src_off[i] + srcs[i0 + i].row0;
        descs[i].mid = c.mid.as<uint8_t>() + mid_off[i];
    }
    // one upload of everything that is not pixels: pool | descriptors | tile prefix of each pass
    const size_t pool_b = up16(pool.size() * 4), desc_b = up16(descs.size() * sizeof(ImgDesc)), pre_b = up16((size_t)(nb + 1) * 4);
    c.meta_host.resize(pool_b + desc_b + 2 * pre_b);
    memcpy(c.meta_host.data(), pool.data(), pool.size() * 4);
    memcpy(c.meta_host.data() + pool_b, descs.data(), descs.size() * sizeof(ImgDesc));
    memcpy(c.meta_host.data() + pool_b + desc_b, pre_h.data(), (size_t)(nb + 1) * 4);
    memcpy(c.meta_host.data() + pool_b + desc_b + pre_b, pre_v.data(), (size_t)(nb + 1) * 4);
    if (c.meta.ensure(c.meta_host.size())) return -1;
    const int32_t* pool_dev = c.meta.as<int32_t>();
    const ImgDesc* descs_dev = reinterpret_cast<const ImgDesc*>(c.meta.as<uint8_t>() + pool_b);
    const unsigned* pre_h_dev = reinterpret_cast<const unsigned*>(c.meta.as<uint8_t>() + pool_b + desc_b);
    const unsigned* pre_v_dev = reinterpret_cast<const unsigned*>(c.meta.as<uint8_t>() + pool_b + desc_b + pre_b);
    MSE_HIP_TRY(hipEventRecord(c.ev[0], st));
    for (int i = 0; i < nb; i++)
        MSE_HIP_TRY(hipMemcpyAsync(c.src.as<uint8_t>() + src_off[i], srcs[i0 + i].data, srcs[i0 + i].bytes, hipMemcpyHostToDevice, st));
    MSE_HIP_TRY(hipMemcpyAsync(c.meta.p, c.meta_host.data(), c.meta_host.size(), hipMemcpyHostToDevice, st));
    MSE_HIP_TRY(hipEventRecord(c.ev[1], st));
    if (pre_h[nb]) {
        hipLaunchKernelGGL(resize_h_kernel, dim3(pre_h[nb]), dim3(H_THREADS), (size_t)seg_cap + (size_t)coef_cap * 4, st, descs_dev, pre_h_dev, nb,
                           pool_dev, out_w, seg_cap, coef_cap);
        MSE_HIP_TRY(hipGetLastError());
    }
    MSE_HIP_TRY(hipEventRecord(c.ev[2], st));
    if (epi == EPI_U8_HWC) {
        hipLaunchKernelGGL(resize_v_kernel<EPI_U8_HWC>, dim3(pre_v[nb]), dim3(V_THREADS), 0, st, descs_dev, pre_v_dev, nb, pool_dev, out_w, out_h,
                           c.out.p);
    } else {
        void* d16 = reinterpret_cast<uint16_t*>(dst) + i0 * out_img;
        hipLaunchKernelGGL(resize_v_kernel<EPI_NCHW_F16>, dim3(pre_v[nb]), dim3(V_THREADS), 0, st, descs_dev, pre_v_dev, nb, pool_dev, out_w,
                           out_h, d16);
    }
    MSE_HIP_TRY(hipGetLastError());
    MSE_HIP_TRY(hipEventRecord(c.ev[3], st));
    if (epi == EPI_U8_HWC)
        MSE_HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint8_t*>(dst) + i0 * out_img, c.out.p, out_img * nb, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));   // the staging is reused by the next sub-batch, the host vectors end here
    for (int k = 0; k < 3; k++) {
        float ms = 0.0f;
        MSE_HIP_TRY(hipEventElapsedTime(&ms, c.ev[k], c.ev[k + 1]));
        c.ms[k] += ms;
        c.ms[3] += ms;
    }
    return 0;
}

}  // namespace

Context::~Context() {
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (own_stream && stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
}

std::shared_ptr<Context> make_context(hipStream_t stream) {
    auto c = std::make_shared<Context>();
    if (stream) {
        c->stream = stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { fail("resize: hipStreamCreate failed"); return nullptr; }
        c->own_stream = true;
    }
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) { fail("resize: hipEventCreate failed"); return nullptr; }
    return c;
}

int run(Context& c, const std::vector<HostSrc>& srcs, int out_w, int out_h, int filter, Epilogue epi, void* dst) {
    for (double& v : c.ms) v = 0.0;
    size_t i0 = 0;
    int rc = 0;
    while (i0 < srcs.size() && !rc) {
        size_t i1 = i0, bytes = 0;
        std::set<TableKey> have;
        while (i1 < srcs.size() && i1 - i0 < (size_t)SUB_BATCH_IMAGES) {
            const size_t b = image_cost(srcs[i1], out_w, out_h, filter, epi, have);
            if (i1 > i0 && bytes + b > STAGE_BYTES) break;
            bytes += b;
            i1++;
        }
        rc = run_sub(c, srcs, i0, i1, out_w, out_h, filter, epi, dst);
        i0 = i1;
    }
    if (rc) (void)hipStreamSynchronize(c.stream);   // nothing of a failed call stays in flight over the caller's memory
    std::lock_guard<std::mutex> lock(g_timing_mu);
    for (int k = 0; k < 4; k++) g_timing[k] = c.ms[k];
    return rc;
}

void last_timing(double ms[4]) {
    std::lock_guard<std::mutex> lock(g_timing_mu);
    for (int k = 0; k < 4; k++) ms[k] = g_timing[k];
}

}  // namespace resize
}  // namespace mse
