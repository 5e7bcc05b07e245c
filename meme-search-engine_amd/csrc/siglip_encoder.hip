// Host side shared by the SigLIP towers: weight store, block weights, block stack (siglip_encoder.h).
#include "siglip_encoder.h"

namespace mse {
namespace siglip {

void Encoder::add_blocks(int depth, const BlockNames& n) {
    const size_t D_ = D, M = mlp, MP = mlp_pad, DP = dp;
    blocks.resize(depth);
    for (int i = 0; i < depth; i++) {
        Block& b = blocks[i];
        const std::string p = n.prefix + std::to_string(i) + ".";
        add_f32(p + n.ln1_g, &b.ln1_g, 1, D_); add_f32(p + n.ln1_b, &b.ln1_b, 1, D_);
        add_bf16(p + n.wqkv, &b.wqkv, 3 * D_, D_, 3 * D_, D_); add_f32(p + n.bqkv, &b.bqkv, 1, 3 * D_);
        // proj and fc2 write the residual branch: their N = D output columns are padded to whole 256-column tiles (zero weight
        // rows, ld DP) so that the persistent 256 x 256 kernel covers them without the half-efficiency 128-column remainder launch
        add_bf16(p + n.wproj, &b.wproj, D_, D_, DP, D_); add_f32(p + n.bproj, &b.bproj, 1, D_, DP);
        add_f32(p + n.ln2_g, &b.ln2_g, 1, D_); add_f32(p + n.ln2_b, &b.ln2_b, 1, D_);
        add_bf16(p + n.w1, &b.w1, M, D_, MP, D_); add_f32(p + n.b1, &b.b1, 1, M, MP);
        add_bf16(p + n.w2, &b.w2, D_, M, DP, MP); add_f32(p + n.b2, &b.b2, 1, D_, DP);
    }
}

bool Encoder::alloc_fused() {
    const size_t D_ = D, MP = mlp_pad;
    bool ok = true;
    for (Block& b : blocks) {
        b.wqkv16 = dalloc<uint16_t>(3 * D_ * D_); b.cqkv = dalloc<float>(3 * D_); b.bqkv2 = dalloc<float>(3 * D_);
        b.w116 = dalloc<uint16_t>(MP * D_); b.c1 = dalloc<float>(MP); b.b12 = dalloc<float>(MP);
        ok = ok && b.wqkv16 && b.cqkv && b.bqkv2 && b.w116 && b.c1 && b.b12;
    }
    ln_stats = dalloc<float>(2 * m_pad, true);
    ln_part = dalloc<float>(2 * (D_ / 64) * m_pad, true);
    sink = dalloc<char>(4096, true);
    return ok && ln_stats && ln_part && sink;
}

const char* Encoder::weight_name(int idx) const {
    if (idx < 0 || idx >= (int)slots.size()) return nullptr;
    auto it = slots.begin();
    std::advance(it, idx);
    return it->first.c_str();
}

int Encoder::set_weight(const char* name, const float* data, const size_t* shape, int ndim) {
    auto it = slots.find(name);
    if (it == slots.end()) return fail(std::string(what) + ": unknown weight '" + name + "'");
    Slot& s = it->second;
    size_t total = 1;
    for (int i = 0; i < ndim; i++) total *= shape[i];
    if (total != s.rows * s.cols) return fail(std::string(what) + ": wrong size for '" + name + "'");
    if (stage_elems < total) {
        if (stage) (void)hipFree(stage);
        stage = nullptr;
        MSE_HIP_TRY(hipMalloc((void**)&stage, total * 4));
        stage_elems = total;
    }
    MSE_HIP_TRY(hipMemcpyAsync(stage, data, total * 4, hipMemcpyHostToDevice, stream));
    if (!s.bf16) {
        if (s.cols_pad == s.cols) MSE_HIP_TRY(hipMemcpyAsync(s.dst, stage, total * 4, hipMemcpyDeviceToDevice, stream));
        else MSE_HIP_TRY(hipMemcpy2DAsync(s.dst, s.cols_pad * 4, stage, s.cols * 4, s.cols * 4, s.rows, hipMemcpyDeviceToDevice, stream));
    } else if (launch_f32_to_bf16_pad(stage, (int)s.rows, (int)s.cols, (int)s.cols, reinterpret_cast<uint16_t*>(s.dst), (int)s.rows_pad,
                                      (int)s.cols_pad, stream)) {
        return -1;
    }
    MSE_HIP_TRY(hipStreamSynchronize(stream));
    s.loaded = true;
    finalized = false;
    return 0;
}

int Encoder::check_loaded() const {
    for (auto& kv : slots)
        if (!kv.second.loaded) return fail(std::string(what) + ": weight '" + kv.first + "' was never set");
    return 0;
}

int Encoder::fold_layernorms() {
    for (int i = 0; fused && i < (int)blocks.size(); i++) {
        Block& b = blocks[i];
        if (launch_ln_fold(b.wqkv, 3 * D, D, b.ln1_g, b.ln1_b, b.bqkv, b.wqkv16, b.cqkv, b.bqkv2, stream)) return -1;
        if (launch_ln_fold(b.w1, mlp_pad, D, b.ln2_g, b.ln2_b, b.b1, b.w116, b.c1, b.b12, stream)) return -1;
    }
    return 0;
}

// The rows of the range are rows b0 * n_pad .. of every activation buffer, its (sequence, head) matrices b0 * H .. of the attention
// operands: a range is an offset into each of them.
int run_blocks(const Encoder& e, const BlockRun& r, hipStream_t st, LnDelta* last) {
    const int D = e.D, MP = e.mlp_pad, depth = (int)e.blocks.size();
    const size_t r0 = (size_t)r.b0 * e.n_pad, bh0 = (size_t)r.b0 * e.H;
    const int M = r.nb * e.n_pad;   // rows incl. the (finite, never read as keys) padding rows of every sequence
    const int Mp = (int)round_up(M, 256);
    uint16_t *x = e.x + r0 * D, *h = e.h + r0 * D, *mlp_h = e.mlp_h + r0 * MP;
    uint16_t* qb = e.qb + bh0 * e.n_pad * e.dh_pad;
    uint16_t* kb = e.kb + bh0 * e.n_pad * attention_k_stride();
    uint16_t* vtb = e.vtb + bh0 * e.dv_pad * e.n_pad;
    auto qkv = [&](GemmLaunch& g) {
        g.M = Mp; g.N = 3 * D; g.K = D; g.m_valid = M; g.tokens = e.n_pad;
        g.q = qb; g.k = kb; g.vt = vtb; g.heads = e.H; g.dh = e.dh; g.dh_pad = e.dh_pad; g.n_pad = e.n_pad;
        g.dv_pad = e.dv_pad; g.kdh_pad = attention_k_stride();
    };
    auto attention = [&]() {
        return launch_attention(qb, kb, vtb, r.nb, e.H, r.tokens, e.n_pad, e.dh, e.dh_pad, e.dv_pad, h, D, e.n_pad, st);
    };
    *last = LnDelta();
    if (r.fused) {
        // LN1 / LN2 folded into the GEMMs around them: proj / fc2 add their tile to the fp16 residual stream in place and emit per-row
        // (sum, M2) of their 64-column groups; QKV / fc1 read the residual rows themselves against gamma-folded weights and correct
        // with (mean, 1/std).  No LayerNorm pass, no bf16 round trip of the branch, no 128-column remainder launch behind proj / fc2.
        float* ln_stats = e.ln_stats + 2 * r0;
        float* ln_part = e.ln_part + 2 * r0;
        auto resid_ln = [&](GemmLaunch& g) {   // x += branch, statistics for the next LayerNorm
            g.M = Mp; g.N = e.dp; g.m_valid = M;
            g.xres = x; g.ldr = D; g.part = ln_part; g.part_rows = e.m_pad; g.n_valid = D; g.sink = e.sink;
            return launch_gemm_fused(GEMM_EPI_RESID_LN, g, st);
        };
        if (launch_row_stats(x, D, D, (size_t)Mp, e.eps, ln_stats, st)) return -1;
        for (int i = 0; i < depth; i++) {  // Encoder1DBlock (model.py:26-44)
            const Block& b = e.blocks[i];
            {
                GemmLaunch g; g.x = x; g.w = b.wqkv16; g.bias = b.bqkv2; g.csum = b.cqkv; g.ln_stats = ln_stats;
                qkv(g);
                if (launch_gemm_fused(GEMM_EPI_QKV, g, st)) return -1;
            }
            if (attention()) return -1;
            {
                GemmLaunch g; g.x = h; g.w = b.wproj; g.bias = b.bproj; g.K = D;
                if (resid_ln(g)) return -1;
            }
            if (launch_ln_finalize(ln_part, e.m_pad, D / 64, (size_t)Mp, e.eps, ln_stats, st)) return -1;
            {
                GemmLaunch g; g.x = x; g.w = b.w116; g.bias = b.b12; g.csum = b.c1; g.ln_stats = ln_stats;
                g.M = Mp; g.N = MP; g.K = D; g.m_valid = M; g.out_bf16 = mlp_h; g.ldo = MP; g.gelu_tanh = e.gelu_tanh;
                if (launch_gemm_fused(GEMM_EPI_GELU, g, st)) return -1;
            }
            {
                GemmLaunch g; g.x = mlp_h; g.w = b.w2; g.bias = b.b2; g.K = MP;
                if (resid_ln(g)) return -1;
            }
            if (i + 1 < depth && launch_ln_finalize(ln_part, e.m_pad, D / 64, (size_t)Mp, e.eps, ln_stats, st)) return -1;
        }
        return 0;
    }
    // Unfused: every LayerNorm a pass of its own that adds the preceding branch to x.  Few rows may split proj / fc2 along K across
    // workgroups; their partial sums and bias are then added by the LayerNorm that consumes the branch (gemm_small_ksplit).
    uint16_t* dlt = e.dlt + r0 * r.ld_branch;
    auto k_split = [&](int ksp) {   // the branch as the LayerNorm behind a GEMM of `ksp` K ranges reads it (bias filled in by the caller)
        LnDelta d;
        if (ksp > 1) { d.parts = e.kparts; d.n_parts = ksp; d.part_stride = r.kpart_stride; d.ldp = D; }
        else { d.bf16 = dlt; d.ldd = r.ld_branch; }
        return d;
    };
    auto branch = [&](GemmLaunch& g, int ksp) {   // proj / fc2: the residual branch, added to x by the next LayerNorm
        g.M = Mp; g.N = r.n_branch; g.m_valid = M; g.out_bf16 = dlt; g.ldo = r.ld_branch; g.skinny = r.skinny;
        g.side = r.side; g.ev_fork = r.side_fork; g.ev_join = r.side_join;
        if (ksp > 1) { g.kpart = e.kparts; g.kpart_stride = r.kpart_stride; g.ksplit = ksp; g.ldr = D; }
        return launch_gemm(ksp > 1 ? GEMM_EPI_PART : GEMM_EPI_BF16, g, st);
    };
    const LnDelta fc2_delta = k_split(r.ksp_fc2);
    for (int i = 0; i < depth; i++) {  // Encoder1DBlock (model.py:26-44)
        const Block& b = e.blocks[i];
        LnDelta d1;   // x += (fc2 output of the previous block), then LayerNorm
        if (i) { d1 = fc2_delta; d1.bias = e.blocks[i - 1].b2; }
        if (launch_layernorm_d(x, 1, D, d1, b.ln1_g, b.ln1_b, e.eps, D, M, h, D, nullptr, r.ln_wg, st)) return -1;
        {
            GemmLaunch g; g.x = h; g.w = b.wqkv; g.bias = b.bqkv; g.skinny = r.skinny;
            g.side = r.side; g.ev_fork = r.side_fork; g.ev_join = r.side_join;
            qkv(g);
            if (launch_gemm(GEMM_EPI_QKV, g, st)) return -1;
        }
        if (attention()) return -1;
        {
            GemmLaunch g; g.x = h; g.w = b.wproj; g.bias = b.bproj; g.K = D;
            if (branch(g, r.ksp_proj)) return -1;
        }
        LnDelta d2 = k_split(r.ksp_proj);   // x += attention branch, then LayerNorm
        if (r.ksp_proj > 1) d2.bias = b.bproj;
        if (launch_layernorm_d(x, 1, D, d2, b.ln2_g, b.ln2_b, e.eps, D, M, h, D, nullptr, r.ln_wg, st)) return -1;
        {
            GemmLaunch g; g.x = h; g.w = b.w1; g.bias = b.b1; g.M = Mp; g.N = MP; g.K = D; g.m_valid = M;
            g.out_bf16 = mlp_h; g.ldo = MP; g.gelu_tanh = e.gelu_tanh; g.skinny = r.skinny;
            if (launch_gemm(GEMM_EPI_GELU, g, st)) return -1;
        }
        {
            GemmLaunch g; g.x = mlp_h; g.w = b.w2; g.bias = b.b2; g.K = MP;
            if (branch(g, r.ksp_fc2)) return -1;
        }
    }
    if (depth) { *last = fc2_delta; last->bias = e.blocks[depth - 1].b2; }
    return 0;
}

}  // namespace siglip
}  // namespace mse
