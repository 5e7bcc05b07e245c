"""The device resize, measured.  Not part of bench.py, not a test.

  python3 scripts/resize_probe.py [--batch 128] [--sizes 1024x768,4000x3000] [--reps 9] [--server-requests 24] [--no-server]

On one MI355X, per source size a batch of `batch` decoded RGB images (eight distinct random images, repeated) resized to 384 x 384:
the wall time of the whole mse_resize_rgb8 call (upload from pageable host memory, both passes, download of the u8 result into a
fresh array) -- one warm-up call, then `reps` calls, EVERY sample kept, median and minimum quoted -- the
HIP-event time of the upload and of each pass alone in those same calls (mse_resize_timing) with the bytes each pass has to move (source + intermediate
for the horizontal pass, intermediate + result for the vertical pass) as GB/s next to the device-to-device copy rate measured in the
same run, and the same batch through Pillow (Image.resize, the same filters) on 16 host threads, timed the same way (warm pool, `reps` samples).  Then the server: images/s of
mse.clip_server.ClipServer's two stages (preprocessing thread, model thread; no HTTP) for requests of 1024 x 768 BMPs with
`device_resize` on, next to requests of 128 BMPs of 384 x 384 through the untouched path, same engine, same run.
Writes profiles/resize_probe.json and prints it; a figure that was not taken reads "not measured yet"."""
import argparse
import asyncio
import json
import os
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  -- before libmse_hip.so

from mse import ffi, siglip  # noqa: E402

OUT = 384
NOT_MEASURED = "not measured yet"


def copy_rate_gbs():
    """device-to-device copy of 1 GiB: bytes read + bytes written per second"""
    n = 1 << 30
    a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * n * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9


def bmp24(rgb):
    h, w, _ = rgb.shape
    stride = (3 * w + 3) & ~3
    rows = np.zeros((h, stride), np.uint8)
    rows[:, :3 * w] = rgb[::-1, :, ::-1].reshape(h, 3 * w)
    pixels = rows.tobytes()
    return (b"BM" + struct.pack("<IHHI", 54 + len(pixels), 0, 0, 54)
            + struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(pixels), 2835, 2835, 0, 0) + pixels)


def resize_case(w, h, batch, reps, copy_gbs):
    """Both arms the same way: one warm-up call, then `reps` timed calls, every sample kept; the figures quoted are the MEDIAN and the
    minimum.  Per device call also the HIP-event times of that same call, so that a slow call shows where its time went."""
    from PIL import Image
    rng = np.random.default_rng(w * 7 + h)
    distinct = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(8)]
    imgs = [distinct[i % 8] for i in range(batch)]
    got = siglip.resize_rgb8(imgs, OUT)                      # warm-up: code objects, staging buffers
    walls, passes = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        siglip.resize_rgb8(imgs, OUT)
        walls.append((time.perf_counter() - t0) * 1e3)
        passes.append(siglip.resize_timing())
    f = Image.HAMMING if (w > OUT and h > OUT) else Image.LANCZOS
    pil_imgs = [Image.fromarray(a, "RGB") for a in imgs]
    pil = []
    with ThreadPoolExecutor(16) as pool:
        want = list(pool.map(lambda im: np.asarray(im.resize((OUT, OUT), f)), pil_imgs))      # warm-up: the pool's threads
        for _ in range(reps):
            t0 = time.perf_counter()
            list(pool.map(lambda im: np.asarray(im.resize((OUT, OUT), f)), pil_imgs))
            pil.append((time.perf_counter() - t0) * 1e3)
    differing = int(sum((got[i] != want[i]).sum() for i in range(8)))
    src_b, mid_b, out_b = batch * w * h * 3, batch * OUT * h * 3, batch * OUT * OUT * 3
    med = lambda xs: float(np.median(xs))
    up, hz, vt = (med([p[k] for p in passes]) for k in ("upload", "horizontal", "vertical"))
    h_gbs, v_gbs = (src_b + mid_b) / (hz * 1e-3) / 1e9, (mid_b + out_b) / (vt * 1e-3) / 1e9
    return {"source": f"{w}x{h}", "batch": batch, "reps": reps, "source_bytes": src_b,
            "call_wall_ms_all": walls, "call_wall_ms_median": med(walls), "call_wall_ms_min": min(walls),
            "images_per_s_whole_call_median": batch / (med(walls) * 1e-3),
            "device_event_ms_all": [p["total"] for p in passes], "device_event_ms_median": med([p["total"] for p in passes]),
            "wall_minus_device_events_ms_all": [wl - p["total"] for wl, p in zip(walls, passes)],
            "upload_ms_all": [p["upload"] for p in passes], "upload_ms_median": up, "upload_gb_s": src_b / (up * 1e-3) / 1e9,
            "horizontal_ms_all": [p["horizontal"] for p in passes], "horizontal_ms_median": hz, "horizontal_bytes": src_b + mid_b,
            "horizontal_gb_s": h_gbs, "horizontal_share_of_copy_rate": h_gbs / copy_gbs,
            "vertical_ms_all": [p["vertical"] for p in passes], "vertical_ms_median": vt, "vertical_bytes": mid_b + out_b,
            "vertical_gb_s": v_gbs, "vertical_share_of_copy_rate": v_gbs / copy_gbs,
            "pillow_16_threads_ms_all": pil, "pillow_16_threads_ms_median": med(pil), "pillow_16_threads_ms_min": min(pil),
            "pillow_16_threads_images_per_s_median": batch / (med(pil) * 1e-3),
            "bytes_differing_from_pillow_first_8_images": differing}


def server_rate(eng, device_resize, files_per_request, requests, file_of):
    """images/s through ClipServer's two stages (threads started, jobs submitted as the POST handler does), no HTTP"""
    from mse.clip_server import ClipServer, Job
    srv = ClipServer({"device": "cuda:0", "model": "ViT-SO400M-14-SigLIP-384", "model_name": "siglip-so400m-14-384",
                      "max_batch_size": files_per_request, "port": 0, "device_resize": device_resize}, eng)
    bodies = [[file_of(r * files_per_request + i) for i in range(files_per_request)] for r in range(min(requests, 4))]

    async def go():
        loop = asyncio.get_running_loop()

        async def one(r):
            job = Job(None, bodies[r % len(bodies)], loop)
            while True:
                try:
                    srv.submit(job)
                    break
                except Exception:  # queue.Full: the handler would answer 500; the probe waits instead
                    await asyncio.sleep(0.001)
            ok, payload = await job.done
            assert ok, payload
            return len(payload)
        await one(0)                                           # warm-up
        t0 = time.perf_counter()
        sem = asyncio.Semaphore(6)

        async def bounded(r):
            async with sem:
                return await one(r)
        n = sum(await asyncio.gather(*[bounded(r) for r in range(requests)]))
        return n / (time.perf_counter() - t0)

    srv.start_threads()
    try:
        return asyncio.new_event_loop().run_until_complete(go())
    finally:
        srv.stop_threads()
        for t in srv._threads:
            t.join(30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--sizes", default="1024x768,4000x3000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--server-requests", type=int, default=24)
    ap.add_argument("--no-server", action="store_true")
    args = ap.parse_args()
    if ffi.lib().mse_device_count() <= 0:
        raise SystemExit("resize_probe: no HIP device visible (nothing is measured without one)")
    ffi.check(ffi.lib().mse_set_device(0))
    copy_gbs = copy_rate_gbs()
    out = {"device_copy_gb_s_read_plus_write": copy_gbs, "output": f"{OUT}x{OUT}", "cases": [], "server": NOT_MEASURED}
    for s in args.sizes.split(","):
        w, h = (int(v) for v in s.split("x"))
        out["cases"].append(resize_case(w, h, args.batch, args.reps, copy_gbs))
    if not args.no_server:
        cfg = dict(siglip.SO400M_384)
        eng = siglip.SiglipImageEngine.from_state_dict(siglip.synthetic_state_dict(cfg), cfg, max_batch=128)
        eng.image_size = (OUT, OUT)
        rng = np.random.default_rng(5)
        big = [bmp24(rng.integers(0, 256, size=(768, 1024, 3), dtype=np.uint8)) for _ in range(8)]
        small = [bmp24(rng.integers(0, 256, size=(OUT, OUT, 3), dtype=np.uint8)) for _ in range(8)]
        # 24 BMPs of 1024 x 768 are 56.6 MB: what fits a request body of the reference's 64 MiB limit
        on = server_rate(eng, True, 24, args.server_requests * 4, lambda i: big[i % 8])
        on128 = server_rate(eng, True, 128, args.server_requests, lambda i: big[i % 8])
        base = server_rate(eng, False, 128, args.server_requests, lambda i: small[i % 8])
        out["server"] = {"what": "ClipServer preprocessing + model stages, one engine, no HTTP, 6 requests in flight, full SO400M tower (synthetic weights)",
                         "device_resize_1024x768_bmp_24_per_request_images_per_s": on,
                         "device_resize_1024x768_bmp_128_per_request_images_per_s": on128,
                         "bmp_384_128_per_request_images_per_s": base, "ratio_24_per_request": on / base, "ratio_128_per_request": on128 / base}
        eng.close()
    path = os.path.join(ROOT, "profiles", "resize_probe.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
