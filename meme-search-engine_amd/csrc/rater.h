// Launchers of rater.hip for rater_api.hip.  Every pointer is a device pointer; every launch goes to `st` and does not wait.
#pragma once
#include "runtime.h"
#include "sae_train.h"   // SaeAdamStep, SaeAdam: the AdamW of DESIGN.md 3.27 step 8, unchanged

namespace mse {

constexpr size_t RATER_MAX_BATCH = 64, RATER_MAX_CHANNELS = 8, RATER_MAX_MEMBERS = 64;

// the words the kernels of a training call share: the gate and what it found
struct RaterCtl {
    uint32_t stop;         // a step was refused: every later kernel of the call returns at once
    uint32_t steps_done;   // completed steps of the call
    uint32_t n_invalid;    // not zero: a slot of the step under way holds a non-finite row
    uint32_t pad;
};

// everything one training step touches.  R = 2 B slots per member: slot 2 b is pair b's first row, slot 2 b + 1 its second
struct RaterStep {
    RaterCtl* ctl;
    const SaeAdamStep* hyper;          // this step's entry
    SaeAdam adam;
    int E, M, C, B;
    const uint16_t* rows;              // slot r of member m: rows + tab[m R + r] * E
    const uint32_t* tab;               // [M][R]
    const float* targets;              // [M][B][C]
    float inv_n;                       // (float)(1.0 / (double)(M B C))
    double* loss;                      // this step's slot
    float *u, *h, *du;                 // [M][R][E]
    float* s;                          // [M][R][C]
    float* g;                          // [M][B][C]
    float *up, *m_up, *v_up;           // [M E][E]
    float *bias, *m_bias, *v_bias;     // [M E]
    float *down, *m_down, *v_down;     // [C][M E]
    int n_cu;
};

// u (optional) and h = silu(u) of slots 0 .. R of every member, [M][R][E]: slot r of member m is row tab[m tab_stride + r], or first + r
// where tab is null.  stop (optional): the gate word
void launch_rater_forward(const uint16_t* rows, int E, int M, const uint32_t* tab, size_t tab_stride, size_t first, size_t R, const float* up,
                          const float* bias, float* u_or_null, float* h, const uint32_t* stop_or_null, hipStream_t st);
// s[m s_member + r s_row + c] from h [M][R][E]
void launch_rater_scores(const float* h, const float* down, int E, int M, int C, size_t R, float* s, size_t s_member, size_t s_row,
                         const uint32_t* stop_or_null, hipStream_t st);
// the row check, the head with the loss and the gate, then du, the update of down and the update of bias
void launch_rater_backward(const RaterStep& s, hipStream_t st);
// the dense pass over up and its moments
void launch_rater_update(const RaterStep& s, hipStream_t st);
// out[i] = the largest channel's variance over the members of sig(s[a_i] - s[b_i]); table [n][M][C]
void launch_rater_pair_variance(const float* table, int M, int C, const uint32_t* a_idx, const uint32_t* b_idx, size_t n_pairs, float* out,
                                hipStream_t st);

}  // namespace mse
