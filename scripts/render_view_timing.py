"""Timing of the viewport decoder (smoe_render_view) on the cfg4-sized model (2160x3840 RGB, 16x16 blocks, 4 kernels), beside
the whole-image decoders (smoe_render / smoe_render_blend) at the same scale on the same model in the same run.

    python scripts/render_view_timing.py [--out profiles/render/render_view_timing.txt]

Views: 1080x1920 output samples of a window at 1x, 4x and 8x (the window starts inside a block), and a 135x240 thumbnail of
the whole image; each without blend and with blend = 2.  Whole image: 1x and 4x, and 8x (a 6.4 GB float32 image) if the
device has the memory.  Method of scripts/render_timing.py: after WARM launches of every shape, REPEATS windows between
device events, the windows of the view alternating with those of the whole-image decoder; a window holds enough launches
for about a tenth of a second or more.  Reported: mean and min..max microseconds per launch over the windows, and samples per
second (output positions, not values) from the mean.  Every measurement runs on the device or the script fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, WARM = 5, 3
SHAPE, C, KPD, GRID = (16, 16), 3, [2, 2], (135, 240)
VIEW = (1080, 1920)
BLENDS = [None, 2.0]


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
    return {"us": round(mean, 2), "min_max_us": [round(min(ts), 2), round(max(ts), 2)], "Gsamples_per_s": round(samples / mean * 1e-3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "render_view_timing.txt"))
    args = ap.parse_args()
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    assert torch.cuda.is_available(), "render_view_timing needs the GPU"
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

    def view_fn(window, size, beta):
        tabs = [blk.view_axis(SHAPE[l], GRID[l], length[l], window[l][0], window[l][1], size[l]) for l in range(2)]
        first, starts = [t[0] for t in tabs], [t[2] for t in tabs]
        axes = [torch.from_numpy(t[3]).cuda() for t in tabs]
        out = torch.empty(tuple(size) + (C,), dtype=torch.float32, device="cuda")
        return (lambda: eng.render_view(dp, act, GRID, first, starts, axes, blend=beta, out=out)), out

    def whole_fn(sc, beta):
        m = [sc * n for n in SHAPE]
        extent = [g * v for g, v in zip(GRID, m)]
        axes = [torch.from_numpy(blk.render_axis(SHAPE[l], m[l])).cuda() for l in range(2)]
        out = torch.empty(tuple(extent) + (C,), dtype=torch.float32, device="cuda")
        if beta is None:
            return (lambda: eng.render(dp, act, axes, GRID, extent, out=out)), out, extent
        return (lambda: eng.render_blend(dp, act, axes, GRID, extent, beta, out=out)), out, extent

    for sc in (1, 4, 8):
        # a window of VIEW / sc source pixels that starts 5 pixels into a block, aligned to the sample pitch
        lo = [533.0, 965.0]
        window = [(lo[l], lo[l] + VIEW[l] / sc) for l in range(2)]
        need = 4 * C * np.prod([g * n * sc for g, n in zip(GRID, SHAPE)])
        fits = torch.cuda.mem_get_info()[0] > 1.5 * need
        for beta in BLENDS:
            vf, vout = view_fn(window, VIEW, beta)
            wf = wout = None
            if fits:
                wf, wout, extent = whole_fn(sc, beta)
            for _ in range(WARM):
                vf()
                if wf:
                    wf()
            torch.cuda.synchronize()
            if wf:                                         # the view is the crop of the whole image, bit for bit
                i0, j0 = int(lo[0] * sc), int(lo[1] * sc)
                same = bool(torch.equal(vout, wout[i0:i0 + VIEW[0], j0:j0 + VIEW[1]]))
            nv, nw = _launches(vf, torch), (_launches(wf, torch) if wf else 0)
            tv, tw = [], []
            for _ in range(REPEATS):
                tv.append(_window(vf, torch, nv))
                if wf:
                    tw.append(_window(wf, torch, nw))
            rec = {"scale": sc, "blend": 0.0 if beta is None else beta, "view": list(VIEW), "window": window,
                   "view_launches_per_window": nv, "render_view": _stats(tv, VIEW[0] * VIEW[1])}
            if wf:
                name = "render" if beta is None else "render_blend"
                rec["whole_extent"] = extent
                rec["whole_launches_per_window"] = nw
                rec[name] = _stats(tw, extent[0] * extent[1])
                rec["view_over_whole_samples_per_s"] = round(rec["render_view"]["Gsamples_per_s"] / rec[name]["Gsamples_per_s"], 3)
                rec["view_equals_crop"] = same
            else:
                rec["whole"] = "not measured: the image does not fit the device memory"
            emit(rec)
            del vout, wout, vf, wf
            torch.cuda.empty_cache()
    for beta in BLENDS:
        size = list(GRID)
        vf, vout = view_fn([(0.0, float(length[0])), (0.0, float(length[1]))], size, beta)
        for _ in range(WARM):
            vf()
        torch.cuda.synchronize()
        nv = _launches(vf, torch)
        tv = [_window(vf, torch, nv) for _ in range(REPEATS)]
        emit({"thumbnail": size, "blend": 0.0 if beta is None else beta, "view_launches_per_window": nv,
              "render_view": _stats(tv, size[0] * size[1])})
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("scripts/render_view_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_render_view on the cfg4-sized model "
                "(2160x3840 RGB, 16x16 blocks, 4 kernels, float32 output), beside smoe_render / smoe_render_blend of the whole image at\n"
                "the same scale in the same run.  us: mean per launch over %d windows (min..max); Gsamples_per_s: output positions per "
                "second from the mean.\n" % REPEATS)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
