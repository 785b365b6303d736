"""Timing of the seam-free decoder (smoe_render_blend) against smoe_render on the same blocks and grid, and what blending buys
on a fitted continuous image.

    python scripts/render_blend_timing.py                  # every timing case, each in a child process under a time limit
    python scripts/render_blend_timing.py --case cfg4
    python scripts/render_blend_timing.py --quality        # PSNR and seam steps of a fitted ramp-plus-edge image, per fit of
                                                           # QUALITY_FITS in a child process under a time limit

Timing: the method of scripts/render_timing.py -- REPEATS windows of LAUNCHES launches between device events, the smoe_render
windows alternating with the smoe_render_blend ones (blend = 0, 1, 2); mean and min..max over the windows.  ``evals`` is the
arithmetic yardstick: the mean number of block evaluations per sample, prod_l (1 + 2 blend_l / n_l)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAUNCHES, REPEATS, WARM = 100, 5, 10
# name: block shape, C, kernels per dim, block grid, scales
CASES = {
    "gray65536": ((16, 16), 1, [2, 2], (256, 256), [1, 2, 4]),
    "cfg4": ((16, 16), 3, [2, 2], (135, 240), [1, 2, 4]),
    "cfg3": ((32, 32), 3, [2, 4], (34, 60), [1, 2, 4]),
}
LIMITS = {"gray65536": 300, "cfg4": 300, "cfg3": 240}
BLENDS = [0.0, 1.0, 2.0]


def _window(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES          # us per launch


def run_case(name):
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    shape, C, kpd, grid, scales = CASES[name]
    B, K = int(np.prod(grid)), int(np.prod(kpd))
    blocks = blk.synthetic_blocks(B, shape, C, 7)
    p0 = blk.init_block_params(blocks, kpd)
    eng = BlockEngine(EngineConfig(block_shape=shape, channels=C, kernels=K, use_yuv=(C == 3), quantize_pis=True))
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    for sc in scales:
        m = [sc * n for n in shape]
        extent = [g * v for g, v in zip(grid, m)]
        axes = [torch.from_numpy(blk.render_axis(shape[l], m[l])).cuda() for l in range(len(shape))]
        out = torch.empty(tuple(extent) + (C,), dtype=torch.float32, device="cuda")

        def ren():
            eng.render(dp, act, axes, grid, extent, out=out)

        def make(beta):
            return lambda: eng.render_blend(dp, act, axes, grid, extent, beta, out=out)

        fns = [make(b) for b in BLENDS]
        for _ in range(WARM):
            ren()
            for f in fns:
                f()
        torch.cuda.synchronize()
        tr, tb = [], [[] for _ in BLENDS]
        for _ in range(REPEATS):
            for i, f in enumerate(fns):
                tr.append(_window(ren, torch))
                tb[i].append(_window(f, torch))
        rec = {"case": name, "blocks": B, "scale": sc, "samples_per_block": m, "extent": extent,
               "render_us": round(float(np.mean(tr)), 2), "render_min_max_us": [round(min(tr), 2), round(max(tr), 2)]}
        for beta, t in zip(BLENDS, tb):
            key = "blend%g" % beta
            rec[key + "_us"] = round(float(np.mean(t)), 2)
            rec[key + "_min_max_us"] = [round(min(t), 2), round(max(t), 2)]
            rec[key + "_ratio"] = round(float(np.mean(t) / np.mean(tr)), 3)
            rec[key + "_ratio_min_max"] = [round(min(t) / max(tr), 3), round(max(t) / min(tr), 3)]
            rec[key + "_evals"] = round(float(np.prod([1 + 2 * beta / n for n in shape])), 3)
        print(json.dumps(rec), flush=True)
    eng.close()


def continuous_image(h=256, w=256):
    """A smooth ramp plus one oblique edge that crosses many blocks (uint8 lattice, as an image file would hold it)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = 0.20 + 0.30 * x / (w - 1) + 0.10 * np.sin(2 * np.pi * y / h)
    edge = 0.25 / (1 + np.exp(-(x - 0.45 * w - 0.37 * (y - h / 2)) / 1.5))
    return (np.rint(np.clip(ramp + edge, 0, 1) * 255) / 255).astype(np.float32)[..., None]


QUALITY_FITS = [(1e-2, 200), (1e-2, 1000)]     # (steering learning rate, iterations)
QUALITY_LIMIT = 240


def run_quality(lr_steer, iters):
    """One fit of the continuous image and its renders.  lr_steer = 1e-2 is the well-conditioned steering rate of bench.py's
    parity section (the reference CLI's default, 1.0, does not give a usable 200-iteration fit of this image)."""
    from steered_mixture_of_experts_amd.smoe import Adam, Smoe
    img = continuous_image()
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=[2, 2], batch_size=[16, 16], use_determinant=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(lr_steer))
    s.train(iters, val_iter=iters)
    s.get_reconstruction()
    n = 16
    for beta in (0.0, 1.0, 2.0):
        rec = {"image": "ramp + oblique edge 256x256", "blocks": "16x16", "iterations": iters, "lr_steer": lr_steer, "blend": beta}
        for sc in (1, 4):
            out = s.render(scale=sc, blend=beta)[..., 0].astype(np.float64)
            if sc == 1:
                mse = float(np.mean((out - img[..., 0]) ** 2))
                rec["psnr_1x_dB"] = round(-10 * np.log10(mse), 3)
            p = n * sc
            steps = [np.abs(np.diff(out, axis=0)), np.abs(np.diff(out, axis=1)).T]      # [j]: between samples j and j + 1
            seam = np.concatenate([st[p - 1::p].ravel() for st in steps])
            mask = np.ones(steps[0].shape[0], bool)
            mask[p - 1::p] = False
            inner = np.concatenate([st[mask].ravel() for st in steps])
            rec["seam_step_%dx" % sc] = round(float(seam.mean()), 6)
            rec["interior_step_%dx" % sc] = round(float(inner.mean()), 6)
            rec["seam_over_interior_%dx" % sc] = round(float(seam.mean() / inner.mean()), 3)
        print(json.dumps(rec), flush=True)


def _children(arg_lists, limits):
    """every case in a child process of its own under a time limit; stops at the first failure"""
    for extra, limit in zip(arg_lists, limits):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, timeout=limit).returncode
        if rc != 0:
            print(f"{' '.join(extra)} failed with exit status {rc}: stopping", flush=True)
            sys.exit(rc if rc > 0 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--fit", type=int, default=None, help="one entry of QUALITY_FITS (what --quality starts per fit)")
    args = ap.parse_args()
    if args.fit is not None:
        return run_quality(*QUALITY_FITS[args.fit])
    if args.quality:
        return _children([["--fit", str(i)] for i in range(len(QUALITY_FITS))], [QUALITY_LIMIT] * len(QUALITY_FITS))
    if args.case:
        return run_case(args.case)
    _children([["--case", name] for name in CASES], [LIMITS[name] for name in CASES])


if __name__ == "__main__":
    main()
