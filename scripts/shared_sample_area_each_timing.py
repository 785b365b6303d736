"""Timing of the area-averaged decoder of whole-image models with per-point footprints (smoe_shared_sample_area_each:
SharedSmoe.eval_points_area_each, eval_projective, eval_map) on the two whole-image models of
profiles/render/shared_sample_timing.txt (512x512 / K = 144 and 2160x3840 RGB / K = 3 840, lists after a 20-iteration fit).

    timeout -k 10 400 python scripts/shared_sample_area_each_timing.py --only a && \
    timeout -k 10 300 python scripts/shared_sample_area_each_timing.py --only b && \
    SMOE_HIP_LIBRARY=<another build> timeout -k 10 200 python scripts/shared_sample_area_each_timing.py --only c --points 32 --ppl 2

Every GPU step under a time limit of its own: --only a writes the file, b and c append to it.

(a) The fused call beside what the tree could do for the same result before it: the valid taps of every sample materialised on
the device (blocks.area_taps_each's arithmetic, made once outside the windows), smoe_shared_sample_grad(want_values) on all of
them, the masked sums per sample (index_add), the division and the lattice in torch.  Views of scripts/sample_area_each_timing.py
sized to the model (1080x1920 samples for the large one, 270x480 for the small one), taps = footprint_taps_each: the tilted view
(0.35 L / E source pixels per sample at the near edge, 1 / 0.09 times that along the tilt at the far edge, where the view
leaves the image) and the barrel-distortion map x = L / 2 + (L / E)(c - E / 2)(1 + 0.3 r^2).  The timed run confirms that the
counts agree exactly and that the fused mean is BIT-IDENTICAL to the ordered tap-by-tap sum of the composition's values.
(b) One footprint broadcast to every point beside smoe_shared_sample_area on the three views of
scripts/shared_sample_area_timing.py; the outputs are bit-identical in the timed run.
(c) The fused call alone on (a)'s views, for a build with other SSE_POINTS / SSE_PPL (--points, --ppl label the lines and
drive the workgroup statistics): run once per build in one session.
Workgroup statistics (from the taps' batches): rounds per workgroup and batch visits per workgroup -- the distinct batches
among a round's items, summed over the rounds -- mean and maximum: what a workgroup walks.
Method of scripts/sample_area_timing.py: after WARM launches, REPEATS windows between device events, the windows of the two
ways alternating; reported are the median and min..max microseconds per call.  Every measurement runs on the device or the
script fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from sample_area_timing import REPEATS, _measure, _stats  # noqa: E402
from shared_sample_timing import FIT  # noqa: E402


def _device_taps_each(torch, pts, foot, taps):
    """blocks.area_taps_each on the device, the valid slots only, in (point, slot) order: positions [T, d], the owner and the
    slot of every tap [T].  The offsets come from the host table of the kernel's divisions; product and sum are separate
    float32 operations."""
    N, d = pts.shape
    n = taps.to(torch.int64)
    void = ((n < 1) | (n > 16)).any(dim=1) | (n.clamp(0, 255).prod(dim=1) > 64) | ~torch.isfinite(foot).all(dim=2).all(dim=1)
    n = torch.where(void[:, None], torch.ones_like(n), n)
    t = torch.arange(64, device="cuda")[None, :]
    valid = (t < n.prod(dim=1)[:, None]) & ~void[:, None]
    owner, slot = valid.nonzero(as_tuple=True)
    nn = np.arange(1, 17)[:, None]
    jj = np.arange(16)[None, :]
    tab = torch.from_numpy(np.where(jj < nn, (2 * jj + 1 - nn).astype(np.float32) / (2 * nn).astype(np.float32), 0).astype(np.float32)).cuda()
    r, nv, off = slot.clone(), n[owner], [None] * d
    for m in range(d - 1, -1, -1):
        off[m] = tab[nv[:, m] - 1, r % nv[:, m]]
        r = r // nv[:, m]
    cols = []
    for l in range(d):
        v = pts[owner, l]
        for m in range(d):
            v = v + foot[owner, l, m] * off[m]
        cols.append(v)
    return torch.stack(cols, dim=-1).contiguous(), owner, slot


def _workgroups(torch, owner, bk, n, points, tile, NB):
    """rounds and batch visits per workgroup of `points` points working through rounds of `tile` items"""
    W = -(-n // points)
    wg = owner // points
    first = torch.searchsorted(wg, torch.arange(W, device="cuda"))             # the taps are in (point, slot) order
    item = torch.arange(owner.shape[0], device="cuda") - first[wg]
    items = torch.bincount(wg, minlength=W)
    rounds = (items + tile - 1) // tile
    ins = bk >= 0
    key = torch.unique((wg[ins] * 64 + item[ins] // tile) * NB + bk[ins].to(torch.int64))
    visits = torch.bincount(key // (64 * NB), minlength=W).to(torch.float32)
    return {"rounds_per_workgroup_mean_max": [round(float(rounds.to(torch.float32).mean()), 2), int(rounds.max())],
            "batch_visits_per_workgroup_mean_max": [round(float(visits.mean()), 2), int(visits.max())]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "shared_sample_area_each_timing.txt"))
    ap.add_argument("--only", choices=["a", "b", "c"], required=True)
    ap.add_argument("--cases", default="shared512,shared2160")
    ap.add_argument("--points", type=int, default=64, help="SSE_POINTS of the library under test")
    ap.add_argument("--ppl", type=int, default=1, help="SSE_PPL of the library under test on two axes (both models have two)")
    args = ap.parse_args()
    import torch
    from render_timing import SHARED_CASES, _shared_image
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import SharedConfig, SharedEngine
    from steered_mixture_of_experts_amd.smoe import footprint_taps_each_torch, map_footprints_torch
    assert torch.cuda.is_available(), "shared_sample_area_each_timing needs the GPU"
    tile = 256 * args.ppl
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for name in args.cases.split(","):
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
        NB = eng.num_batches
        head = {"model": name, "SSE_POINTS": args.points, "SSE_PPL": args.ppl, "batches": NB, "kernels": K}
        L = np.array(shape, dtype=np.float64)
        E = (1080, 1920) if shape[0] >= 2160 else (270, 480)

        def views():
            z = 0.35 * L / np.array(E)
            H = np.array([[z[0], -0.7 / E[1] * L[0] / 2, -z[0] * E[0] / 2 + L[0] / 2], [0.0, z[1], 0.0], [0.0, -0.7 / E[1], 1.0]])
            pts, foot, valid = blk.projective_points(H, E)
            assert valid.all()
            yield "tilted view %dx%d" % E, torch.from_numpy(pts.reshape(-1, 2)).cuda(), torch.from_numpy(foot.reshape(-1, 2, 2)).cuda()
            c = np.stack(np.meshgrid(*[np.arange(e, dtype=np.float64) + 0.5 - e / 2 for e in E], indexing="ij"), axis=-1)
            r2 = (c ** 2).sum(axis=-1) / ((np.array(E) / 2) ** 2).sum()
            bar = torch.from_numpy((L / 2 + (L / np.array(E)) * c * (1.0 + 0.3 * r2)[..., None]).astype(np.float32)).cuda()
            yield "barrel map %dx%d, k = 0.3" % E, bar.reshape(-1, 2).contiguous(), map_footprints_torch(bar).reshape(-1, 2, 2).contiguous()

        def against_composition(label, pts, foot, fused_only):
            taps = footprint_taps_each_torch(foot)
            n = int(pts.shape[0])
            tap_dev, owner, slot = _device_taps_each(torch, pts, foot, taps)
            nt = int(tap_dev.shape[0])
            out = torch.empty((n, C), dtype=torch.float32, device="cuda")
            held = {}

            def fused():
                held["fused"] = eng.sample_area_each(dp, lists, pts, foot, taps, out=out, want_mean=True, want_count=True)

            tn = taps.to(torch.int64).prod(dim=1)
            rec = dict(head, case=label, samples=n, taps=nt, taps_per_sample_mean_max=[round(nt / n, 2), int(tn.max())],
                       tap_tuples=int(torch.unique(taps, dim=0).shape[0]))
            if fused_only:
                ts = _measure({"shared_sample_area_each": fused}, torch)
                rec.update({k: _stats(v, nt) for k, v in ts.items()})
                _, _, bk = eng.sample_grad(dp, lists, tap_dev, want_values=True, want_batch=True)
            else:
                jac = torch.empty((nt, 2, C), dtype=torch.float32, device="cuda")

                def composed():
                    _, val, bk = eng.sample_grad(dp, lists, tap_dev, out=jac, want_values=True, want_batch=True)
                    ins = bk >= 0
                    cnt = torch.zeros((n,), dtype=torch.float32, device="cuda").index_add_(0, owner, ins.to(torch.float32))
                    total = torch.zeros((n, C), dtype=torch.float32, device="cuda").index_add_(0, owner, val * ins[:, None])
                    mean = torch.where(cnt[:, None] > 0, total / cnt.clamp(min=1)[:, None], torch.zeros_like(total))
                    held["composed"] = (torch.floor(mean * 255.0 + 0.5) / 255.0, mean, cnt, val, bk)

                ts = _measure({"shared_sample_area_each": fused, "shared_sample_grad_and_torch_mean": composed}, torch)
                rec.update({k: _stats(v, nt) for k, v in ts.items()})
                rec["composition_over_fused_time"] = round(rec["shared_sample_grad_and_torch_mean"]["us"] / rec["shared_sample_area_each"]["us"], 3)
                fv, fm, fc = held["fused"]
                cv, cm, cc, val, bk = held["composed"]
                # the mean once more in the stated order, tap by tap: bit for bit the fused one
                acc = torch.zeros((n, C), dtype=torch.float32, device="cuda")
                ins = bk >= 0
                for s in range(int(tn.max())):
                    sel = (slot == s) & ins                                      # at most one tap of a point
                    acc[owner[sel]] = acc[owner[sel]] + val[sel]
                ordered = torch.where(cc[:, None] > 0, acc / cc.clamp(min=1)[:, None], torch.zeros_like(acc))
                rec["taps_inside_share"] = round(float(fc.to(torch.float32).sum()) / nt, 4)
                rec["counts_equal"] = bool(torch.equal(fc.to(torch.float32), cc))
                rec["mean_bit_identical_to_ordered_composition"] = bool(torch.equal(fm.view(torch.int32), ordered.view(torch.int32)))
                rec["max_abs_difference_to_index_add_mean"] = float((fm - cm).abs().max())
                rec["lattice_values_equal_share"] = round(float(((fv - cv).abs() < 1e-7).float().mean()), 6)
                assert rec["counts_equal"] and rec["mean_bit_identical_to_ordered_composition"] and torch.isfinite(fm).all()
            rec.update(_workgroups(torch, owner, bk, n, args.points, tile, NB))
            emit(rec)
            torch.cuda.empty_cache()

        def against_shared_sample_area(label, A, size, taps):
            F = np.asarray(A, dtype=np.float64)[:, :2].astype(np.float32)
            pts = torch.from_numpy(blk.warp_points(A, size).reshape(-1, 2)).cuda()
            n, nt = int(pts.shape[0]), int(np.prod(taps))
            foot = torch.from_numpy(F).cuda()[None].expand(n, 2, 2).contiguous()
            tp = torch.tensor(taps, dtype=torch.uint8, device="cuda")[None].expand(n, 2).contiguous()
            o1 = torch.empty((n, C), dtype=torch.float32, device="cuda")
            o2 = torch.empty((n, C), dtype=torch.float32, device="cuda")
            held = {}

            def one():
                held["one"] = eng.sample_area(dp, lists, pts, F, taps, out=o1, want_mean=True, want_count=True, want_batch=True)

            def each():
                held["each"] = eng.sample_area_each(dp, lists, pts, foot, tp, out=o2, want_mean=True, want_count=True, want_batch=True)

            ts = _measure({"shared_sample_area": one, "shared_sample_area_each": each}, torch)
            rec = dict(head, case=label, samples=n, taps="x".join(map(str, taps)), **{k: _stats(v, n * nt) for k, v in ts.items()})
            rec["each_over_one_footprint_time"] = round(rec["shared_sample_area_each"]["us"] / rec["shared_sample_area"]["us"], 3)
            rec["bit_identical"] = all(bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(held["one"], held["each"]))
            assert rec["bit_identical"]
            emit(rec)

        if args.only in ("a", "c"):
            for label, pts, foot in views():
                against_composition(label, pts, foot, args.only == "c")
        else:
            against_shared_sample_area("1/8 thumbnail", [[8, 0, 0], [0, 8, 0]], (shape[0] // 8, shape[1] // 8), (8, 8))
            against_shared_sample_area("1/2 view", [[2, 0, 0], [0, 2, 0]], (shape[0] // 2, shape[1] // 2), (2, 2))
            c17, s17 = 3 * np.cos(np.deg2rad(17.0)), 3 * np.sin(np.deg2rad(17.0))
            M = np.array([[c17, -s17], [s17, c17]])
            E3 = (shape[0] // 3, shape[1] // 3)
            rot = np.concatenate([M, (L / 2 - M @ (np.array(E3, dtype=np.float64) / 2))[:, None]], axis=1)
            against_shared_sample_area("1/3 view rotated by 17 degrees", rot, E3, (3, 3))
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    fresh = args.only == "a"
    with open(args.out, "w" if fresh else "a") as f:
        if fresh:
            f.write("scripts/shared_sample_area_each_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_shared_sample_area_each "
                    "(values, mean, count) on the two models of shared_sample_timing.txt (lists after a %d-iteration fit); (a) beside "
                    "smoe_shared_sample_grad(want_values) on the materialised taps plus the masked sums, the division and the lattice in "
                    "torch, (b) with broadcast footprints beside smoe_shared_sample_area, (c) the fused call alone under other SSE_POINTS / "
                    "SSE_PPL builds.\nus: median per call over %d alternating windows (min..max); Gtaps_per_s: taps per second from the "
                    "median; the ratios are ratios of the medians; the tap list of the composition is made outside its windows; rounds / "
                    "batch visits per workgroup: from the taps' batches, for the SSE_POINTS / SSE_PPL of the line.\n" % (FIT, REPEATS))
        f.write("(%s)\n" % args.only + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
