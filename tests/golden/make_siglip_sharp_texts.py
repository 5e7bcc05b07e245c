"""Token rows for the text tower's end-to-end check with sharpened attention (tests/test_gpu_siglip_attention.py).

That check multiplies the q projection of every block by lambda = 8 and holds the engine to 1e-3 of cosine against the fp32 oracle.  It
says something about the KERNEL only for texts on which the engine's number format alone -- q, k, v rounded to bf16 -- costs the oracle
far less than that (the test asks for at most 1e-4), and only if the lazy running maximum is actually raised late (at least 5 % of the
query rows).  Plain `synthetic_tokens` meets neither well: the text tower reads ONE position of a 64-key softmax, nothing averages a
flipped near-tie away, and 15 of its first 112 texts cost 1e-4 .. 2.2e-4; and a text whose real tokens end before key 32 has only copies
of the pad token in its second half, which never raise a maximum (0.1 % of the rows of texts shorter than 16, 12 % for 48 and more).

So, from the same generator: texts with MORE than 32 real tokens (a structural condition, taken first), of those the ones whose bf16
cost in the oracle is at most 5e-5 -- half of what the test asks, because the cost of one text moves by up to 3e-5 with the batch it
is computed in (fp32 GEMM blocking) -- the first 112 in generator order.  Nothing the engine computes enters the choice.

Run from the repo root:  python tests/golden/make_siglip_sharp_texts.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import siglip_ref as ref  # noqa: E402
import test_gpu_siglip_attention as t  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "siglip_sharp_texts.npz")
N, POOL, SEEDS, MIN_REAL, MAX_COST, LAMBDA = 112, 112, range(0x5EED0B00, 0x5EED0B10), 33, 5e-5, 8


def main():
    torch.set_grad_enabled(False)
    cfg = dict(ref.TEXT_CONFIG, layers=t.DEPTH)
    sd = t.sharpen(ref.synthetic_text_weights(cfg), t.text_names(), LAMBDA)
    kept, seen = [], 0
    for seed in SEEDS:
        tok = ref.synthetic_tokens(POOL, cfg, seed=seed)
        tok = tok[(tok != 1).sum(1) >= MIN_REAL]
        cost = 1 - t.cosine(ref.encode_text(tok, sd, cfg).numpy(), ref.encode_text(tok, sd, cfg, qkv_hook=t.round_qkv).numpy())
        seen += len(tok)
        kept += [tok[i].numpy() for i in np.flatnonzero(cost <= MAX_COST)]
        print("seed %#x: %d texts of %d or more real tokens, %d at most %.0e (median %.2e, largest %.2e); kept so far %d" %
              (seed, len(tok), MIN_REAL, int((cost <= MAX_COST).sum()), MAX_COST, np.median(cost), cost.max(), len(kept)))
        if len(kept) >= N:
            break
    assert len(kept) >= N, len(kept)
    tokens = np.stack(kept[:N]).astype(np.int32)
    np.savez_compressed(OUT, tokens=tokens, lam=LAMBDA, min_real=MIN_REAL, max_cost=MAX_COST, considered=seen)
    print("wrote", OUT, tokens.shape, "from", seen, "considered")


if __name__ == "__main__":
    main()
