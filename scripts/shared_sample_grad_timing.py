"""Timing of the shared-mode point derivative (smoe_shared_sample_grad / smoe_shared_render_view_grad: SharedSmoe.eval_points_grad,
eval_view_grad, eval_warp_grad) on the two whole-image models of profiles/render/shared_sample_timing.txt, beside
smoe_shared_sample / smoe_shared_render_view on the same points in the same run.

    python scripts/shared_sample_grad_timing.py [--out profiles/render/shared_sample_grad_timing.txt] [--cases shared512,shared2160]

Per model (set up as scripts/shared_sample_timing.py does: lists after a 20-iteration fit): (a) every pixel centre of the image as
a row-major point list; (b) the whole image as a view at 1x; (c) the central quarter-by-quarter window at 4x; (d) a view of the
image's size rotated by 30 degrees about the centre at zoom 1.5; (e) 4096 scattered probes.  Every line has the derivative
(Jacobian and values stored) and the value decoder on the same points, their windows alternating (the method of
scripts/shared_sample_timing.py: WARM launches, REPEATS windows between device events, a window about a tenth of a second);
reported are the median per launch, the spread (min .. max of the windows) and the ratio of the medians, beside the ratio of
the bytes stored, (d C + C) / C.  Every measurement runs on the device or the script fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from shared_sample_timing import DEG, FIT, PROBES, REPEATS, ZOOM, _measure  # noqa: E402


def _stats(ts):
    return {"median_us": round(float(np.median(ts)), 2), "min_max_us": [round(min(ts), 2), round(max(ts), 2)]}


def run_case(name, emit):
    import torch
    from render_timing import SHARED_CASES, _shared_image
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import SharedConfig, SharedEngine
    shape, bs, C, kpd, _ = SHARED_CASES[name]
    d = len(shape)
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
    head = {"model": name, "batches": eng.num_batches, "kernels": K, "mean_list_length": round(mean_len, 1),
            "stored_bytes_ratio": round((d * C + C) / C, 2)}

    def points_fns(host):
        pts = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda()
        n = pts.shape[0]
        out = torch.empty((n, C), dtype=torch.float32, device="cuda")
        jac = torch.empty((n, d, C), dtype=torch.float32, device="cuda")
        return {"grad": lambda: eng.sample_grad(dp, lists, pts, out=jac, want_values=True),
                "value": lambda: eng.sample(dp, lists, pts, out=out)}

    def view_fns(win, E):
        axes, batches = [], []
        for l in range(d):
            axes.append(torch.from_numpy(blk.view_axis(shape[l], 1, shape[l], win[l][0], win[l][1], E[l])[3]).cuda())
            first, nblocks, start, _ = blk.view_axis(bs[l], shape[l] // bs[l], shape[l], win[l][0], win[l][1], E[l])
            batches.append(torch.from_numpy((first + np.repeat(np.arange(nblocks), np.diff(start))).astype(np.int32)).cuda())
        out = torch.empty(tuple(E) + (C,), dtype=torch.float32, device="cuda")
        jac = torch.empty(tuple(E) + (d, C), dtype=torch.float32, device="cuda")
        return {"grad": lambda: eng.render_view_grad(dp, lists, axes, batches, out=jac, want_values=True),
                "value": lambda: eng.render_view(dp, lists, axes, batches, out=out)}

    def line(case, fns, samples):
        ts = _measure(fns, torch)
        rec = dict(head, case=case, samples=samples, **{k: _stats(v) for k, v in ts.items()})
        rec["grad_over_value_time"] = round(rec["grad"]["median_us"] / rec["value"]["median_us"], 3)
        emit(rec)

    centres = blk.warp_points([[1, 0, 0], [0, 1, 0]], shape).reshape(-1, 2)
    line("every pixel centre as points, row-major", points_fns(centres), N)
    line("the whole image as a view at 1x", view_fns([(0.0, float(s)) for s in shape], shape), N)
    line("the central quarter window at 4x", view_fns([(3 * s / 8, 5 * s / 8) for s in shape], shape), N)
    c, s = np.cos(np.deg2rad(DEG)) / ZOOM, np.sin(np.deg2rad(DEG)) / ZOOM
    M = np.array([[c, -s], [s, c]])
    A = np.concatenate([M, (np.array(shape) / 2 - M @ (np.array(shape) / 2))[:, None]], axis=1)
    line("a view of the image's size rotated by 30 degrees at zoom 1.5", points_fns(blk.warp_points(A, shape).reshape(-1, 2)), N)
    probes = np.random.default_rng(2).uniform(0.0, 1.0, size=(PROBES, 2)) * np.array(shape)
    line("%d scattered probes" % PROBES, points_fns(probes), PROBES)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "shared_sample_grad_timing.txt"))
    ap.add_argument("--cases", default="shared512,shared2160")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "shared_sample_grad_timing needs the GPU"
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for name in args.cases.split(","):
        run_case(name, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("scripts/shared_sample_grad_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_shared_sample_grad / "
                "smoe_shared_render_view_grad (Jacobian and values stored) beside smoe_shared_sample / smoe_shared_render_view on the "
                "same points in the same run, the two models of shared_sample_timing.txt (lists after a %d-iteration fit).\n"
                "median_us: median per launch over %d alternating windows (min..max: the spread); grad_over_value_time: ratio of "
                "the medians; stored_bytes_ratio: (d C + C) / C.\n" % (FIT, REPEATS))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
