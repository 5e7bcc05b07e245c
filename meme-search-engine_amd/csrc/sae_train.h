// Launchers of sae_train.hip for sae_train_api.hip.  Every pointer is a device pointer; every launch goes to `st` and does not wait.
#pragma once
#include "runtime.h"

namespace mse {

constexpr size_t SAE_TRAIN_MAX_PAIRS = 65536;   // batch * top_k of one step

// what one step's AdamW needs besides the betas and eps, computed in double on the host (uploaded as a table, one entry per step)
struct SaeAdamStep { float decay, step_size, bc2_sqrt; };

// the words the kernels of a call share: the gate and what it found
struct SaeTrainCtl {
    uint32_t stop;         // a step was refused: every later kernel of the call returns at once
    uint32_t steps_done;   // completed steps of the call
    uint32_t n_pairs;      // kept (row, feature) pairs of the step under way
    uint32_t n_invalid;    // sae_merge_kernel's count of invalid rows of the step under way
};

struct SaeAdam { float beta1, beta2, eps; };

// everything one step's backward pass and update touch
struct SaeTrainStep {
    SaeTrainCtl* ctl;
    const SaeAdamStep* hyper;          // this step's entry
    SaeAdam adam;
    int B, E, H, K;
    // the forward pass's outputs
    const uint32_t *counts, *feats;    // [B], [B][K]
    const float *acts, *recon;         // [B][K], [B][E]
    const double* sqerr;               // [B]
    const uint16_t* rows;              // source row i: rows + (ids ? ids[i] : first + i) * E
    const uint32_t* ids;
    size_t first;
    double* loss;                      // this step's slot
    // the step's own scratch
    float* gR;                         // [B][E]
    uint32_t *p_row, *p_feat;          // [B K] the pairs in (feature, row) order
    float *p_act, *p_h;
    uint2* fmap;                       // [H] member range of each feature, {0, 0} between steps
    uint8_t* touched;                  // [H] the feature has had a member since the moments were zero
    int skip;                          // rows of up / downT that were never touched may be skipped (decay == 1)
    // parameters and moments
    float *up, *m_up, *v_up, *downT, *m_down, *v_down;   // [H][E]
    float *up_bias, *m_ub, *v_ub;                        // [H] or null
    float *down_bias, *m_db, *v_db;                      // [E]
    unsigned long long* counters;                        // [H]
    int n_cu;
};

// the gate, the loss and the pair count of a step (after the forward pass)
void launch_sae_train_gate(const SaeTrainStep& s, hipStream_t st);
// the pair index, gR with the decoder bias's gradient and update, the hidden gradients, the encoder bias's update, the counters
void launch_sae_train_backward(const SaeTrainStep& s, hipStream_t st);
// the dense pass over up and downT and their moments, then the member map is cleared
void launch_sae_train_update(const SaeTrainStep& s, hipStream_t st);

}  // namespace mse
