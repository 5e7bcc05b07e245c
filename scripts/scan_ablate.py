"""Developer timing of the MFMA scan kernel alone (HIP events around the kernel): python scripts/scan_ablate.py [rows] [queries]
MSE_SCAN_ABL=<bits> selects an ablated variant of the 256-query kernel (scan_mfma.hip); results are then meaningless.
MSE_SCAN_MID=0..4 selects the schedule of the 320-query search kernel (0: without the mid-block barrier; scan_mfma.hip MID), with
MSE_SCAN_ABL=33 its stamped form: the K block split into issue, mid-block barrier, closing wait and closing barrier, and the clock held."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MSE_HIP_LIB", os.path.join(ROOT, "meme-search-engine_amd", "lib", "libmse_hip_dev.so"))   # developer library (make dev)
sys.path.insert(0, os.path.join(ROOT, "meme-search-engine_amd"))
import torch  # noqa: F401,E402
import mse  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 256
if os.environ.get("ZERO_X"):   # power / DVFS probe: same traffic, operands that do not toggle the multipliers
    zt = torch.zeros(n * 1152, dtype=torch.float16, device="cuda")
    if os.environ["ZERO_X"] == "2":
        zt.fill_(1.0)
    torch.cuda.synchronize()
    vl = mse.VectorList.wrap_device(zt.data_ptr(), n, 1152, keepalive=zt)
else:
    vl = mse.VectorList.generate(0x5EED0001, 0, n)
qs = mse.VectorList.generate(0x5EED0002, 0, nq)
s = mse.Searcher(vl)
if os.environ.get("SPARSE"):   # the 320-query pass: thresholded group maxima off | auto | forced (Searcher.set_sparse_maxima)
    s.set_sparse_maxima(os.environ["SPARSE"], int(os.environ.get("SPARSE_STRIDE", 0)))
out_s = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
out_i = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
for _ in range(2):
    s.bruteforce_topk_dev(qs.device_ptr, nq, 10, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA)
s.scan_timing(2)
t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
import time
t0 = time.perf_counter()
for _ in range(5):
    s.bruteforce_topk_dev(qs.device_ptr, nq, 10, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA)
torch.cuda.synchronize()
wall = (time.perf_counter() - t0) / 5
ms, k = s.scan_timing(0)
print(f"2d={os.environ.get('MSE_SCAN_2D', '-')} abl={os.environ.get('MSE_SCAN_ABL', '0')} S={os.environ.get('MSE_SCAN_S', '3')} rows={n} nq={nq}: scan {ms / k:.3f} ms "
      f"({n * 2304 / (ms / k) / 1e6:.0f} GB/s), step {wall * 1e3:.3f} ms")
if os.environ.get("CHECK") and os.environ.get("MSE_SCAN_2D") != "162":   # the variant's answers against the exact-order kernel (first 8 queries)
    chk_s = torch.empty((8, 10), dtype=torch.int64, device="cuda")
    chk_i = torch.empty((8, 10), dtype=torch.int32, device="cuda")
    s.bruteforce_topk_dev(qs.device_ptr, 8, 10, chk_s.data_ptr(), chk_i.data_ptr(), mse.MODE_EXACT)
    torch.cuda.synchronize()
    print("answers equal the exact-order kernel:", bool(torch.equal(chk_s, out_s[:8]) and torch.equal(chk_i, out_i[:8])), s.last_stats())
if os.environ.get("MSE_SCAN_2D") == "161" or os.environ.get("MSE_SCAN_ABL") == "33":   # developer library: where a wave's cycles go (scan_mfma.hip, PROF)
    import ctypes
    from mse import ffi
    out = (ctypes.c_ulonglong * 7)()
    ffi.lib().mse_dev_scan_prof(out)          # clear what the warm-up and the timed loop left
    s.scan_timing(2)
    REPS = 5                                  # back to back, so that the clock figure below is not that of a chip waking up
    for _ in range(REPS):
        s.bruteforce_topk_dev(qs.device_ptr, nq, 10, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA)
    torch.cuda.synchronize()
    ffi.lib().mse_dev_scan_prof(out)
    issue, wait, bar, nkb, turn, tiles, mid = [int(x) // REPS for x in out]
    tot = issue + wait + bar + mid
    print(f"profiled 2-D scan (MSE_SCAN_MID={os.environ.get('MSE_SCAN_MID', 'product')}): per K block and wave {tot / nkb:.0f} cycles = issue {issue / nkb:.0f}"
          f" + mid-block barrier {mid / nkb:.0f} + vmcnt wait {wait / nkb:.0f} + barrier {bar / nkb:.0f} ({nkb} wave-K-blocks)")
    # the clock the stamped kernel held: stamped cycles per wave slot (8 waves on each CU, every launch fills the chip at these sizes)
    # over the HIP-event time of the step's scan launches
    ms1, k1 = s.scan_timing(0)
    slots = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    ms1 /= REPS
    print(f"stamped step: scan {ms1:.3f} ms; {(tot + turn) / slots:.0f} stamped cycles per wave slot = {(tot + turn) / slots / ms1 / 1e6:.3f} GHz held")
    if tiles:   # per row tile and wave: its K loop against the turn-over (epilogue + prologue) around it
        print(f"per tile and wave: K loop {tot / tiles:.0f} cycles ({nkb / tiles:.1f} K blocks) + turn-over {turn / tiles:.0f} cycles = "
              f"{turn / (tot + turn) * 100:.2f} % of the tile ({tiles} wave-tiles, sparse maxima {os.environ.get('SPARSE', 'auto')})")
