"""Timing of the area-averaged point decoder (smoe_sample_area) on the cfg4-sized model (2160x3840 RGB, 16x16 blocks, 4 kernels),
beside what the tree could do for the same result before it: every tap materialised as a point, smoe_sample_grad(want_values)
on all of them, the masked mean and the lattice in torch.

    python scripts/sample_area_timing.py [--out profiles/render/sample_area_timing.txt]

Views: (a) a 1/8 thumbnail of the whole image, 270x480 samples of 8x8 taps; (b) a 1/2 view, 1080x1920 samples of 2x2 taps;
(c) a 1/3 view rotated by 17 degrees about the image centre, 720x1280 samples of 3x3 taps (its corners leave the image: their
taps are left out of the mean); each without blend and with blend = 2.  Every view has 8.3 M taps.
Method of scripts/sample_timing.py: after WARM launches of every shape, REPEATS windows between device events, the windows of
the two ways alternating; a window holds enough launches for about a tenth of a second or more.  Reported: median and min..max
microseconds per call over the windows, taps per second from the median, and the time ratio composition / fused.  The tap list
of the composition is made once, outside its windows, and its cost is reported apart: on the host (blocks.area_taps and the
upload, wall clock) and on the device (the same arithmetic in torch, device events; compared bit for bit with the host's).
In the timed run the composition's mean is compared with the fused mean (the torch sum associates differently: a few ulps) and
its lattice image with the fused values.  Every measurement runs on the device or the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, WARM = 5, 3
SHAPE, C, KPD, GRID = (16, 16), 3, [2, 2], (135, 240)


def _window(fn, torch, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches           # us per call


def _launches(fn, torch):
    """calls per window: about 0.15 s of work, at least 3"""
    t = _window(fn, torch, 3)
    return int(min(2000, max(3, 150e3 / max(t, 1.0))))


def _stats(ts, taps):
    med = float(np.median(ts))
    return {"us": round(med, 2), "min_max_us": [round(min(ts), 2), round(max(ts), 2)], "Gtaps_per_s": round(taps / med * 1e-3, 3)}


def _measure(fns, torch):
    """alternating windows of the given calls: {name: [us per call]}"""
    for _ in range(WARM):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    n = {k: _launches(f, torch) for k, f in fns.items()}
    ts = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, f in fns.items():
            ts[k].append(_window(f, torch, n[k]))
    return ts


def _device_taps(torch, pts, F, taps):
    """blocks.area_taps in torch on the device: the same float32 operations in the same order"""
    d = pts.shape[1]
    off = [(torch.arange(n, device="cuda", dtype=torch.float32) * 2 + (1 - n)) / float(2 * n) for n in taps]
    jj = torch.cartesian_prod(*[torch.arange(n, device="cuda") for n in taps]).reshape(-1, d)
    cols = []
    for l in range(d):
        t = pts[:, l:l + 1].expand(-1, jj.shape[0])
        for m in range(d):
            t = t + (off[m][jj[:, m]] * float(F[l, m]))[None, :]
        cols.append(t)
    return torch.stack(cols, dim=-1).reshape(-1, d).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "sample_area_timing.txt"))
    args = ap.parse_args()
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    assert torch.cuda.is_available(), "sample_area_timing needs the GPU"
    os.environ.pop("SMOE_SAMPLE_RECORDS", None)
    B, K = int(np.prod(GRID)), int(np.prod(KPD))
    length = [g * n for g, n in zip(GRID, SHAPE)]
    p0 = blk.init_block_params(blk.synthetic_blocks(B, SHAPE, C, 7), KPD)
    eng = BlockEngine(EngineConfig(block_shape=SHAPE, channels=C, kernels=K, use_yuv=True, quantize_pis=True))
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    lines = []

    def case(name, A, size, taps, beta):
        F = np.asarray(A, dtype=np.float64)[:, :2].astype(np.float32)
        host = blk.warp_points(A, size).reshape(-1, 2)
        pts = torch.from_numpy(host).cuda()
        n, nt = int(pts.shape[0]), int(np.prod(taps))
        t0 = time.perf_counter()
        tap_host = blk.area_taps(host, F, taps).reshape(-1, 2)
        tap_dev = torch.from_numpy(tap_host).cuda()
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        gen = _measure({"taps": lambda: _device_taps(torch, pts, F, taps)}, torch)["taps"]
        dev_equal = bool(torch.equal(_device_taps(torch, pts, F, taps).view(torch.int32), tap_dev.view(torch.int32)))
        img = torch.empty((n, C), dtype=torch.float32, device="cuda")
        jac = torch.empty((n * nt, 2, C), dtype=torch.float32, device="cuda")
        held = {}

        def fused():
            held["fused"] = eng.sample_area(dp, act, GRID, length, pts, F, taps, blend=beta, out=img, want_mean=True, want_count=True)

        def composed():
            _, val, bk = eng.sample_grad(dp, act, GRID, length, tap_dev, blend=beta, out=jac, want_values=True, want_block=True)
            ins = (bk >= 0).reshape(n, nt)
            cnt = ins.sum(dim=1)
            total = (val.reshape(n, nt, C) * ins[:, :, None]).sum(dim=1)
            mean = torch.where(cnt[:, None] > 0, total / cnt.clamp(min=1).to(torch.float32)[:, None], torch.zeros_like(total))
            held["composed"] = (torch.floor(mean * 255.0 + 0.5) / 255.0, mean, cnt)

        ts = _measure({"sample_area": fused, "sample_grad_and_torch_mean": composed}, torch)
        rec = {"case": name, "samples": n, "taps": "x".join(map(str, taps)), "blend": 0.0 if beta is None else beta,
               **{k: _stats(v, n * nt) for k, v in ts.items()}}
        rec["composition_over_fused_time"] = round(rec["sample_grad_and_torch_mean"]["us"] / rec["sample_area"]["us"], 3)
        rec["tap_list_on_the_host_ms"] = round(host_ms, 1)
        rec["tap_list_on_the_device_us"] = round(float(np.median(gen)), 2)
        rec["device_tap_list_equals_host"] = dev_equal
        fv, fm, fc = held["fused"]
        cv, cm, cc = held["composed"]
        rec["taps_inside_share"] = round(float(fc.to(torch.float32).mean()) / nt, 4)
        rec["max_abs_mean_difference"] = float((fm - cm).abs().max())
        rec["lattice_values_equal"] = round(float(((fv - cv).abs() < 1e-7).float().mean()), 6)
        assert torch.equal(fc.to(torch.int64), cc) and torch.isfinite(fm).all()
        assert rec["max_abs_mean_difference"] < 1e-5 and rec["lattice_values_equal"] > 0.999
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del img, jac, held, tap_dev
        torch.cuda.empty_cache()

    L = np.array(length, dtype=np.float64)
    c17, s17 = 3 * np.cos(np.deg2rad(17.0)), 3 * np.sin(np.deg2rad(17.0))
    M = np.array([[c17, -s17], [s17, c17]])
    rot = np.concatenate([M, (L / 2 - M @ (np.array([720.0, 1280.0]) / 2))[:, None]], axis=1)
    for beta in (None, 2.0):
        case("1/8 thumbnail", [[8, 0, 0], [0, 8, 0]], (270, 480), (8, 8), beta)
    for beta in (None, 2.0):
        case("1/2 view", [[2, 0, 0], [0, 2, 0]], (1080, 1920), (2, 2), beta)
    for beta in (None, 2.0):
        case("1/3 view rotated by 17 degrees", rot, (720, 1280), (3, 3), beta)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("scripts/sample_area_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_sample_area (values, mean, count) beside "
                "smoe_sample_grad(want_values) on the materialised taps plus the masked mean and the lattice in torch, on the cfg4-sized "
                "model (2160x3840 RGB, 16x16 blocks, 4 kernels).\nus: median per call over %d alternating windows (min..max); Gtaps_per_s: "
                "taps per second from the median; composition_over_fused_time: ratio of the medians; the tap list of the composition is "
                "made outside its windows (tap_list_on_the_host_ms: blocks.area_taps and the upload; tap_list_on_the_device_us: the same "
                "arithmetic in torch).\n" % REPEATS)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
