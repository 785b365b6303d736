"""Timing of the point decoder (smoe_sample) on the cfg4-sized model (2160x3840 RGB, 16x16 blocks, 4 kernels), beside the grid
decoders on the same model in the same run.

    python scripts/sample_timing.py [--out profiles/render/sample_timing.txt]

Cases: (a) every pixel centre of the image as points, against smoe_render at 1x and smoe_render_view of the whole image (the
three give the same image, checked); (b) a 1080x1920 view rotated by 17 degrees at 4x, without blend and with blend = 2;
(c) the points of (b) shuffled -- every workgroup's points span the whole view, so it takes the direct path -- and the points
of (b) in order with SMOE_SAMPLE_RECORDS=0 (nothing staged, whatever the default does); (d) as many random probes inside a
64x64-pixel region (16 blocks: the staged path), against the same probes with SMOE_SAMPLE_RECORDS=0 (the direct path).
Method of scripts/render_view_timing.py: after WARM launches of every shape, REPEATS windows between device events, the
windows of the decoders that are compared alternating; a window holds enough launches for about a tenth of a second or more.  Reported: mean and min..max microseconds per launch over the
windows, points per second from the mean, and the ratios.  Every measurement runs on the device or the script fails."""
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
    mean = float(np.mean(ts))
    return {"us": round(mean, 2), "min_max_us": [round(min(ts), 2), round(max(ts), 2)], "Gpoints_per_s": round(samples / mean * 1e-3, 3)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "sample_timing.txt"))
    args = ap.parse_args()
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    assert torch.cuda.is_available(), "sample_timing needs the GPU"
    os.environ.pop("SMOE_SAMPLE_RECORDS", None)
    B, K = int(np.prod(GRID)), int(np.prod(KPD))
    length = [g * n for g, n in zip(GRID, SHAPE)]
    p0 = blk.init_block_params(blk.synthetic_blocks(B, SHAPE, C, 7), KPD)
    eng = BlockEngine(EngineConfig(block_shape=SHAPE, channels=C, kernels=K, use_yuv=True, quantize_pis=True))
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def sample_fn(pts, beta, records=None):
        out = torch.empty((pts.shape[0], C), dtype=torch.float32, device="cuda")

        def run():
            if records is not None:                        # the hook is read by every call
                os.environ["SMOE_SAMPLE_RECORDS"] = str(records)
            eng.sample(dp, act, GRID, length, pts, blend=beta, out=out)
            if records is not None:
                del os.environ["SMOE_SAMPLE_RECORDS"]
        return run, out

    # (a) every pixel centre, against render at 1x and render_view of the whole image
    N = length[0] * length[1]
    centres = torch.from_numpy(blk.warp_points([[1, 0, 0], [0, 1, 0]], length).reshape(-1, 2)).cuda()
    sf, sout = sample_fn(centres, None)
    axes = [torch.from_numpy(blk.render_axis(SHAPE[l], SHAPE[l])).cuda() for l in range(2)]
    rout = torch.empty(tuple(length) + (C,), dtype=torch.float32, device="cuda")
    rf = lambda: eng.render(dp, act, axes, GRID, length, out=rout)
    tabs = [blk.view_axis(SHAPE[l], GRID[l], length[l], 0.0, float(length[l]), length[l]) for l in range(2)]
    vaxes = [torch.from_numpy(t[3]).cuda() for t in tabs]
    vout = torch.empty(tuple(length) + (C,), dtype=torch.float32, device="cuda")
    vf = lambda: eng.render_view(dp, act, GRID, [t[0] for t in tabs], [t[2] for t in tabs], vaxes, out=vout)
    ts = _measure({"sample": sf, "render": rf, "render_view": vf}, torch)
    rec = {"case": "every pixel centre", "points": N, "blend": 0.0, **{k: _stats(v, N) for k, v in ts.items()}}
    rec["sample_over_render_time"] = round(rec["sample"]["us"] / rec["render"]["us"], 3)
    rec["sample_over_render_view_time"] = round(rec["sample"]["us"] / rec["render_view"]["us"], 3)
    rec["same_image"] = bool(torch.equal(sout.view(rout.shape), rout) and torch.equal(vout, rout))
    emit(rec)
    del centres, sout, rout, vout
    torch.cuda.empty_cache()

    # (b), (c) a rotated 4x view; the axis-aligned 4x view of the same size beside it
    c, s = np.cos(np.deg2rad(DEG)) / ZOOM, np.sin(np.deg2rad(DEG)) / ZOOM
    M = np.array([[c, -s], [s, c]])
    A = np.concatenate([M, (np.array(length) / 2 - M @ (np.array(VIEW) / 2))[:, None]], axis=1)
    host = blk.warp_points(A, VIEW).reshape(-1, 2)
    assert blk.point_blocks(host, SHAPE, GRID, length)[0].all()
    n = host.shape[0]
    rot = torch.from_numpy(host).cuda()
    shuf = rot[torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()].contiguous()
    lo = [(length[l] - VIEW[l] / ZOOM) / 2 for l in range(2)]
    window = [(lo[l], lo[l] + VIEW[l] / ZOOM) for l in range(2)]
    for beta in (None, 2.0):
        tabs = [blk.view_axis(SHAPE[l], GRID[l], length[l], window[l][0], window[l][1], VIEW[l]) for l in range(2)]
        vaxes = [torch.from_numpy(t[3]).cuda() for t in tabs]
        vout = torch.empty(tuple(VIEW) + (C,), dtype=torch.float32, device="cuda")
        vf = lambda: eng.render_view(dp, act, GRID, [t[0] for t in tabs], [t[2] for t in tabs], vaxes, blend=beta, out=vout)
        sf, sout = sample_fn(rot, beta)
        df, dout = sample_fn(rot, beta, records=0)
        hf, hout = sample_fn(shuf, beta)
        ts = _measure({"sample": sf, "sample_records_0": df, "sample_shuffled": hf, "render_view_axis_aligned": vf}, torch)
        rec = {"case": "1080x1920 view rotated by 17 degrees at 4x", "points": n, "blend": 0.0 if beta is None else beta,
               **{k: _stats(v, n) for k, v in ts.items()}}
        rec["sample_over_render_view_time"] = round(rec["sample"]["us"] / rec["render_view_axis_aligned"]["us"], 3)
        rec["records_0_over_default_time"] = round(rec["sample_records_0"]["us"] / rec["sample"]["us"], 3)
        rec["shuffled_over_ordered_time"] = round(rec["sample_shuffled"]["us"] / rec["sample"]["us"], 3)
        rec["records_0_same_bits"] = bool(torch.equal(sout.view(torch.int32), dout.view(torch.int32)))
        emit(rec)
        del vout, sout, dout, hout
        torch.cuda.empty_cache()
    # (d) random probes inside 4 x 4 blocks: every lane changes block from point to point, the box is small
    rng = np.random.default_rng(2)
    probes = torch.from_numpy((rng.uniform(0.0, 64.0, size=(n, 2)) + np.array([944.0, 1680.0])).astype(np.float32)).cuda()
    for beta in (None, 2.0):
        sf, sout = sample_fn(probes, beta)
        df, dout = sample_fn(probes, beta, records=0)
        ts = _measure({"sample": sf, "sample_records_0": df}, torch)
        rec = {"case": "random probes inside 64x64 pixels (4x4 blocks)", "points": n, "blend": 0.0 if beta is None else beta,
               **{k: _stats(v, n) for k, v in ts.items()}}
        rec["records_0_over_default_time"] = round(rec["sample_records_0"]["us"] / rec["sample"]["us"], 3)
        rec["records_0_same_bits"] = bool(torch.equal(sout.view(torch.int32), dout.view(torch.int32)))
        emit(rec)
        del sout, dout
        torch.cuda.empty_cache()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("scripts/sample_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_sample on the cfg4-sized model (2160x3840 RGB, "
                "16x16 blocks, 4 kernels, float32 output), beside smoe_render / smoe_render_view in the same run.\nus: mean per launch "
                "over %d windows (min..max); Gpoints_per_s: points (output positions) per second from the mean; *_time: ratios of the "
                "mean times.\n" % REPEATS)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
