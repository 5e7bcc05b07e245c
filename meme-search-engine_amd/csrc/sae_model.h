// The model handle of sae_api.hip, shared with sae_train_api.hip (the trainer updates its device weights in place).
#pragma once
#include "../../include/mse.h"
#include "sae.h"

struct mse_sae {
    uint64_t serial = 0;         // which model a table was made by (an address can be reused); a training call draws a new one
    uint64_t uid = 0;            // never changes: how a trainer recognises its model among the live ones
    int device = 0, n_cu = 256;
    size_t d_emb = 0, d_hidden = 0, top_k = 0;
    float *up = nullptr, *up_bias = nullptr, *downT = nullptr, *down_bias = nullptr;   // device; downT [d_hidden][d_emb]
    unsigned long long* counters = nullptr;                                           // device [d_hidden]
    int parts = 0;               // mse_sae_set_hidden_parts: 0 = automatic
    std::mutex mu;               // guards the scratch below, the counters and -- against a training call -- the weights
    mse::DevBuf lists, pcount, pflag, misc;   // the parts' candidate lists, lengths and NaN flags; the invalid-row count
};

namespace mse {

constexpr size_t SAE_LIST_BUDGET = (size_t)512 << 20;   // bytes of candidate lists one launch may use

uint64_t sae_next_serial();
// whether m is a live model (mse_sae_load'ed and not yet freed) with that uid
bool sae_model_alive(const mse_sae* m, uint64_t uid);

// hidden parts of a call of n rows: as many workgroups as run at once, two per CU, and no more (workgroups take equally long, so one
// past that number would be a second round); no part without a tile
inline void sae_choose_parts(const mse_sae* m, size_t n, int* parts, int* tiles_per_part) {
    const size_t n_tiles = (m->d_hidden + SAE_HID_TILE - 1) / SAE_HID_TILE, row_tiles = (n + SAE_ROW_TILE - 1) / SAE_ROW_TILE;
    size_t p = m->parts > 0 ? (size_t)m->parts : 2 * (size_t)m->n_cu / row_tiles;
    p = std::max<size_t>(1, std::min<size_t>(p, std::min<size_t>(n_tiles, m->parts > 0 ? SAE_MAX_PARTS : 256)));
    const size_t tpp = (n_tiles + p - 1) / p;
    *tiles_per_part = (int)tpp;
    *parts = (int)((n_tiles + tpp - 1) / tpp);
}

}  // namespace mse
