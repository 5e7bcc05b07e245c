// Host side shared by the SigLIP image and text towers (siglip_api.hip, siglip_text_api.hip): the engine's device memory and
// named weights, the weights of the pre-LN transformer blocks, and the block stack that runs them on the kernels of
// siglip_kernels.hip.  What the towers do differently is passed in by the caller; nothing here asks which tower it serves.
#pragma once
#include "common.h"
#include "siglip.h"
#include <map>
#include <string>
#include <vector>

namespace mse {
namespace siglip {

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

struct Block {
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    uint16_t *wqkv, *wproj, *w1, *w2;
    float *bqkv, *bproj, *b1, *b2;
    // LayerNorm folded into QKV / fc1 (fused path, built by fold_layernorms): fp16 w * gamma, its row sums, bias + w . beta
    uint16_t *wqkv16 = nullptr, *w116 = nullptr;
    float *cqkv = nullptr, *c1 = nullptr, *bqkv2 = nullptr, *b12 = nullptr;
};

// A tower's names of the twelve tensors of block i: prefix + i + "." + the name
struct BlockNames {
    const char *prefix, *ln1_g, *ln1_b, *wqkv, *bqkv, *wproj, *bproj, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
};

struct Slot {
    bool bf16;                  // converted to bf16 and padded; else fp32 with rows of cols_pad
    void* dst;
    size_t rows, cols;          // logical shape of the source (product of leading dims, last dim)
    size_t rows_pad, cols_pad;  // destination shape
    bool loaded = false;
};

// What both towers' engines hold: geometry, device memory, named weights, blocks and the activations of the block stack.
// Token rows of sequence b are rows b * n_pad + t of every [M][..] buffer.
struct Encoder {
    const char* what = "";       // error-message prefix: "siglip" / "siglip text"
    int D = 0, H = 0, dh = 0, mlp = 0, mlp_pad = 0, n_pad = 0, dh_pad = 96, dv_pad = 80;
    int dp = 0;                  // D rounded up to whole 256-column GEMM tiles (rows of the proj / fc2 weights, zero behind D)
    int max_batch = 0;
    size_t m_pad = 0;
    float eps = 0;
    int gelu_tanh = 0;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    std::map<std::string, Slot> slots;   // sorted: the order *_weight_name enumerates
    bool finalized = false;
    float* stage = nullptr; size_t stage_elems = 0;
    std::vector<Block> blocks;
    // fused LayerNorm path (siglip_kernels.hip "Fused LayerNorm"); MSE_SIGLIP_NOFUSE=1 keeps LN1 / LN2 as kernels of their own
    bool fused = false;
    float* ln_stats = nullptr;   // [m_pad] (mean, 1/std)
    float* ln_part = nullptr;    // [D / 64][m_pad] (sum, M2)
    void* sink = nullptr;
    // activations of the block stack
    uint16_t* x = nullptr;       // residual stream [M][D], fp16
    uint16_t *h = nullptr, *dlt = nullptr, *mlp_h = nullptr, *qb = nullptr, *kb = nullptr, *vtb = nullptr;
    float* kparts = nullptr;     // fp32 partial sums of a K-split proj / fc2 (launch_gemm GEMM_EPI_PART)

    Encoder() = default;
    Encoder(const Encoder&) = delete;
    ~Encoder() {   // the streams must be idle
        for (void* p : allocs) (void)hipFree(p);
        if (stage) (void)hipFree(stage);
    }

    template <typename T> T* dalloc(size_t n, bool zero = false) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n * sizeof(T), 256)) != hipSuccess) return nullptr;
        if (zero && hipMemset(p, 0, std::max<size_t>(n * sizeof(T), 256)) != hipSuccess) return nullptr;
        allocs.push_back(p);
        return reinterpret_cast<T*>(p);
    }
    void add_f32(const std::string& name, float** dst, size_t rows, size_t cols, size_t cols_pad = 0) {
        const size_t cp = cols_pad ? cols_pad : cols;
        *dst = dalloc<float>(rows * cp, true);
        slots[name] = Slot{false, *dst, rows, cols, rows, cp};
    }
    void add_bf16(const std::string& name, uint16_t** dst, size_t rows, size_t cols, size_t rows_pad, size_t cols_pad) {
        *dst = dalloc<uint16_t>(rows_pad * cols_pad, true);
        slots[name] = Slot{true, *dst, rows, cols, rows_pad, cols_pad};
    }
    void add_blocks(int depth, const BlockNames& n);
    bool alloc_fused();          // the folded weights of every block and the LayerNorm statistics; false if out of memory
    int n_weights() const { return (int)slots.size(); }
    const char* weight_name(int idx) const;
    int set_weight(const char* name, const float* data, const size_t* shape, int ndim);
    int check_loaded() const;    // fails naming the first weight never set
    int fold_layernorms();       // fused path: launch_ln_fold of LN1 into QKV and of LN2 into fc1, every block, on `stream`
};

// One run of the block stack over the sequences [b0, b0 + nb) and what differs between the towers' runs
struct BlockRun {
    int b0 = 0, nb = 0;
    int tokens = 0;              // attention length (the token stride is n_pad)
    bool fused = false;          // LN1 / LN2 folded into the GEMMs around them
    int skinny = 0;              // unfused: GemmLaunch::skinny of QKV, proj, fc1, fc2
    int ln_wg = 0;               // unfused: launch_layernorm_d's `wg` of LN1 / LN2, decided by the caller for the whole CALL
    int n_branch = 0, ld_branch = 0;   // unfused: output columns of proj / fc2 and the row stride of the branch they write (dlt)
    hipStream_t side = nullptr;        // unfused: GemmLaunch::side (and its events) of QKV, proj, fc2
    hipEvent_t side_fork = nullptr, side_join = nullptr;
    int ksp_proj = 1, ksp_fc2 = 1;     // unfused: K ranges of proj / fc2 (1 = none) ...
    size_t kpart_stride = 0;           // ... and the slab stride of their partial sums in kparts
};

// Enqueues every block on `st`.  `last`: what a LayerNorm after the stack must add to x (the last fc2's branch and bias;
// empty on the fused path, which leaves the whole residual in x).
int run_blocks(const Encoder& e, const BlockRun& r, hipStream_t st, LnDelta* last);

// A range of sequences on a stream of its own, joined back by an event
struct SideRange {
    int b0, nb;
    hipStream_t st;
    hipEvent_t join;
};

// Runs `run(b0, nb, stream, index)` for every side range (forked from `main` by `fork`, enqueued first), then for [0, nb0) on
// `main`, and makes `main` wait for the side ranges.  `index` is 1 + the side range's position, 0 for the main stream's range.
template <typename F>
int fork_join(hipStream_t main, hipEvent_t fork, const std::vector<SideRange>& sides, int nb0, F&& run) {
    if (!sides.empty()) MSE_HIP_TRY(hipEventRecord(fork, main));
    for (size_t i = 0; i < sides.size(); i++) {
        MSE_HIP_TRY(hipStreamWaitEvent(sides[i].st, fork, 0));
        if (run(sides[i].b0, sides[i].nb, sides[i].st, (int)i + 1)) return -1;
        MSE_HIP_TRY(hipEventRecord(sides[i].join, sides[i].st));
    }
    if (run(0, nb0, main, 0)) return -1;
    for (const SideRange& s : sides) MSE_HIP_TRY(hipStreamWaitEvent(main, s.join, 0));
    return 0;
}

}  // namespace siglip
}  // namespace mse
