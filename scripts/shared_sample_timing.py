"""Timing of the shared-mode point and viewport decoders (smoe_shared_sample / smoe_shared_render_view: SharedSmoe.eval_points,
eval_view, eval_warp) on the two whole-image models of profiles/render/shared_render_timing.txt, beside smoe_shared_render of
the same sample count in the same run.

    python scripts/shared_sample_timing.py [--out profiles/render/shared_sample_timing.txt] [--cases shared512,shared2160]

Per model (set up as scripts/render_timing.py does: lists as they are after a short fit): (a) every pixel centre of the image
as a row-major point list; (b) the whole image as a view at 1x, and the central quarter-by-quarter window at 4x (as many
samples as the image has pixels); (c) a view of the image's size rotated by 30 degrees about the centre at zoom 1.5; (d) the
points of (a) shuffled (every workgroup meets as many batches as it has points, or all of them); (e) 4096 scattered probes.
The yardstick beside every line is smoe_shared_render on the training lattice -- the same number of samples as (a) - (d).
Method of scripts/sample_timing.py: after WARM launches of every shape, REPEATS windows between device events, the windows of
the launches that are compared alternating; a window holds enough launches for about a tenth of a second.  The launches are
the engine's (device time per launch; the facade adds the host-side tables and copies).  Every measurement runs on the device
or the script fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

REPEATS, WARM, FIT = 5, 3, 20
DEG, ZOOM, PROBES = 30.0, 1.5, 4096


def _window(fn, torch, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches           # us per launch


def _measure(fns, torch):
    """alternating windows of the given launches: {name: [us per launch]}"""
    for _ in range(WARM):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    n = {k: int(min(2000, max(3, 100e3 / max(_window(f, torch, 3), 1.0)))) for k, f in fns.items()}
    ts = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, f in fns.items():
            ts[k].append(_window(f, torch, n[k]))
    return ts


def _stats(ts, samples):
    mean = float(np.mean(ts))
    return {"us": round(mean, 2), "min_max_us": [round(min(ts), 2), round(max(ts), 2)], "Gsamples_per_s": round(samples / mean * 1e-3, 3)}


def run_case(name, emit):
    import torch
    from render_timing import SHARED_CASES, _shared_image
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import SharedConfig, SharedEngine
    shape, bs, C, kpd, _ = SHARED_CASES[name]
    img = _shared_image(shape, C)
    p0 = {k: v[0] for k, v in blk.init_block_params(img[None], kpd).items()}
    K = int(p0["pis"].shape[0])
    eng = SharedEngine(SharedConfig(image_shape=shape, batch_shape=bs, channels=C, kernels=K, use_yuv=(C == 3)))
    tb, _ = blk.image_to_blocks(img, bs)
    T = torch.from_numpy(blk.to_planar(tb)).cuda()
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    lists = eng.new_lists()
    eng.forward(T, dp, lists, want_recon=False)
    eng.fit(T, dp, eng.new_adam_state(dp), lists, FIT)
    eng.update_kernel_list(dp, lists)
    eng.forward(T, dp, lists, want_recon=False)
    torch.cuda.synchronize()
    words = lists.cpu().numpy().view(np.uint32)
    mean_len = float(np.mean([sum(bin(int(w)).count("1") for w in row) for row in words]))
    N = int(np.prod(shape))
    head = {"model": name, "batches": eng.num_batches, "kernels": K, "mean_list_length": round(mean_len, 1)}

    raxes = [torch.from_numpy(blk.render_axis(s, s)).cuda() for s in shape]
    rout = torch.empty(tuple(shape) + (C,), dtype=torch.float32, device="cuda")
    render = lambda: eng.render(dp, lists, raxes, bs, out=rout)

    def points_fn(host):
        pts = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda()
        out = torch.empty((pts.shape[0], C), dtype=torch.float32, device="cuda")
        return (lambda: eng.sample(dp, lists, pts, out=out)), out

    def view_fn(win, E):
        axes, batches = [], []
        for l in range(2):
            axes.append(torch.from_numpy(blk.view_axis(shape[l], 1, shape[l], win[l][0], win[l][1], E[l])[3]).cuda())
            first, nblocks, start, _ = blk.view_axis(bs[l], shape[l] // bs[l], shape[l], win[l][0], win[l][1], E[l])
            batches.append(torch.from_numpy((first + np.repeat(np.arange(nblocks), np.diff(start))).astype(np.int32)).cuda())
        out = torch.empty(tuple(E) + (C,), dtype=torch.float32, device="cuda")
        return (lambda: eng.render_view(dp, lists, axes, batches, out=out)), out

    def line(case, fns, samples, same=None):
        ts = _measure(dict(fns, shared_render_1x=render), torch)
        rec = dict(head, case=case, samples=samples, **{k: _stats(v, samples if k != "shared_render_1x" else N) for k, v in ts.items()})
        for k in fns:
            rec[k + "_over_render_time"] = round(rec[k]["us"] / rec["shared_render_1x"]["us"], 3)
        if same is not None:
            rec["same_image_as_render"] = bool(same())
        emit(rec)

    centres = blk.warp_points([[1, 0, 0], [0, 1, 0]], shape).reshape(-1, 2)
    pf, pout = points_fn(centres)
    line("every pixel centre as points, row-major", {"sample": pf}, N, lambda: torch.equal(pout.view(rout.shape), rout))
    whole = [(0.0, float(s)) for s in shape]
    vf, vout = view_fn(whole, shape)
    quarter = [(3 * s / 8, 5 * s / 8) for s in shape]
    qf, _ = view_fn(quarter, shape)
    line("views: the whole image at 1x, the central quarter window at 4x", {"view_1x": vf, "view_4x": qf}, N,
         lambda: torch.equal(vout, rout))
    c, s = np.cos(np.deg2rad(DEG)) / ZOOM, np.sin(np.deg2rad(DEG)) / ZOOM
    M = np.array([[c, -s], [s, c]])
    A = np.concatenate([M, (np.array(shape) / 2 - M @ (np.array(shape) / 2))[:, None]], axis=1)
    warp = blk.warp_points(A, shape).reshape(-1, 2)
    wf, _ = points_fn(warp)
    hf, hout = points_fn(centres[np.random.default_rng(1).permutation(N)])
    line("a view of the image's size rotated by 30 degrees at zoom 1.5; the pixel centres shuffled",
         {"sample_warp": wf, "sample_shuffled": hf}, N)
    probes = np.random.default_rng(2).uniform(0.0, 1.0, size=(PROBES, 2)) * np.array(shape)
    sf, _ = points_fn(probes)
    line("%d scattered probes" % PROBES, {"sample_probes": sf}, PROBES)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "shared_sample_timing.txt"))
    ap.add_argument("--cases", default="shared512,shared2160")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "shared_sample_timing needs the GPU"
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for name in args.cases.split(","):
        run_case(name, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("scripts/shared_sample_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_shared_sample / smoe_shared_render_view "
                "on the two models of shared_render_timing.txt (float32 output, lists after a short fit), beside smoe_shared_render on "
                "the training lattice in the same run.\nus: mean per launch over %d windows (min..max); Gsamples_per_s: output positions "
                "per second from the mean; *_over_render_time: ratios of the mean times to shared_render_1x of the same line.\n" % REPEATS)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
