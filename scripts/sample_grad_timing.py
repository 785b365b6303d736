"""Timing of the point derivative (smoe_sample_grad) on the cfg4-sized model (2160x3840 RGB, 16x16 blocks, 4 kernels), beside
smoe_sample on the same points in the same run.

    python scripts/sample_grad_timing.py [--out profiles/render/sample_grad_timing.txt]

Point sets: (a) every pixel centre of the image; (b) a 1080x1920 view rotated by 17 degrees at 4x, without blend and with
blend = 2; (c) the points of (b) shuffled (every workgroup's points span the whole view: the direct path), without and with
blend; (d) as many random probes inside a 64x64-pixel region (16 blocks), without and with blend.
Method of scripts/sample_timing.py: after WARM launches of every shape, REPEATS windows between device events, the windows of
the two decoders alternating; a window holds enough launches for about a tenth of a second or more.  Reported: median and
min..max microseconds per launch over the windows, points per second from the median, and the time ratio grad / sample.
The yardstick is smoe_sample on the same points; the derived mark is the output-byte ratio (d C + C) / C = 1 + d = 3 (the
Jacobian and the values against the values).  In the timed run the values of smoe_sample_grad, put on the lattice, are
compared with smoe_sample's image (share of equal samples; they differ only on rounding ties, tests/test_gpu_sample_grad.py).
Every measurement runs on the device or the script fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, WARM = 5, 3
SHAPE, C, KPD, GRID = (16, 16), 3, [2, 2], (135, 240)
VIEW, DEG, ZOOM = (1080, 1920), 17.0, 4.0


def _window(fn, torch, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches           # us per launch


def _launches(fn, torch):
    """launches per window: about 0.15 s of work, at least 3"""
    t = _window(fn, torch, 3)
    return int(min(2000, max(3, 150e3 / max(t, 1.0))))


def _stats(ts, samples):
    med = float(np.median(ts))
    return {"us": round(med, 2), "min_max_us": [round(min(ts), 2), round(max(ts), 2)], "Gpoints_per_s": round(samples / med * 1e-3, 3)}


def _measure(fns, torch):
    """alternating windows of the given launches: {name: [us per launch]}"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "sample_grad_timing.txt"))
    args = ap.parse_args()
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    assert torch.cuda.is_available(), "sample_grad_timing needs the GPU"
    os.environ.pop("SMOE_SAMPLE_RECORDS", None)
    B, K = int(np.prod(GRID)), int(np.prod(KPD))
    length = [g * n for g, n in zip(GRID, SHAPE)]
    p0 = blk.init_block_params(blk.synthetic_blocks(B, SHAPE, C, 7), KPD)
    eng = BlockEngine(EngineConfig(block_shape=SHAPE, channels=C, kernels=K, use_yuv=True, quantize_pis=True))
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    lines = []

    def case(name, pts, beta):
        n = int(pts.shape[0])
        img = torch.empty((n, C), dtype=torch.float32, device="cuda")
        jac = torch.empty((n, 2, C), dtype=torch.float32, device="cuda")
        holder = {}

        def grad():
            holder["val"] = eng.sample_grad(dp, act, GRID, length, pts, blend=beta, out=jac, want_values=True)[1]
        ts = _measure({"sample_grad": grad, "sample": lambda: eng.sample(dp, act, GRID, length, pts, blend=beta, out=img)}, torch)
        rec = {"case": name, "points": n, "blend": 0.0 if beta is None else beta, **{k: _stats(v, n) for k, v in ts.items()}}
        rec["grad_over_sample_time"] = round(rec["sample_grad"]["us"] / rec["sample"]["us"], 3)
        rec["output_byte_ratio"] = 3.0
        lat = torch.floor(holder["val"].clamp(0.0, 1.0) * 255.0 + 0.5) / 255.0
        rec["values_on_the_lattice_equal_sample"] = round(float(((lat - img).abs() < 1e-7).float().mean()), 6)
        rec["max_abs_jac"] = round(float(jac.abs().max()), 4)
        assert torch.isfinite(jac).all() and rec["values_on_the_lattice_equal_sample"] > 0.999
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del img, jac, holder
        torch.cuda.empty_cache()

    case("every pixel centre", torch.from_numpy(blk.warp_points([[1, 0, 0], [0, 1, 0]], length).reshape(-1, 2)).cuda(), None)
    c, s = np.cos(np.deg2rad(DEG)) / ZOOM, np.sin(np.deg2rad(DEG)) / ZOOM
    M = np.array([[c, -s], [s, c]])
    A = np.concatenate([M, (np.array(length) / 2 - M @ (np.array(VIEW) / 2))[:, None]], axis=1)
    host = blk.warp_points(A, VIEW).reshape(-1, 2)
    assert blk.point_blocks(host, SHAPE, GRID, length)[0].all()
    n = host.shape[0]
    rot = torch.from_numpy(host).cuda()
    shuf = rot[torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()].contiguous()
    probes = torch.from_numpy((np.random.default_rng(2).uniform(0.0, 64.0, size=(n, 2)) + np.array([944.0, 1680.0])).astype(np.float32)).cuda()
    for beta in (None, 2.0):
        case("1080x1920 view rotated by 17 degrees at 4x", rot, beta)
    for beta in (None, 2.0):
        case("the same points shuffled", shuf, beta)
    for beta in (None, 2.0):
        case("random probes inside 64x64 pixels (4x4 blocks)", probes, beta)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("scripts/sample_grad_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_sample_grad (Jacobian [N, 2, 3] + values "
                "[N, 3], float32) beside smoe_sample (values [N, 3], float32) on the same points of the cfg4-sized model (2160x3840 "
                "RGB, 16x16 blocks, 4 kernels).\nus: median per launch over %d alternating windows (min..max); Gpoints_per_s: points per "
                "second from the median; grad_over_sample_time: ratio of the medians, beside the output-byte ratio 1 + d = 3.\n" % REPEATS)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
