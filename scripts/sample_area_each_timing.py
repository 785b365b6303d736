"""Timing of the area-averaged point decoder with per-point footprints (smoe_sample_area_each) on the cfg4-sized model
(2160x3840 RGB, 16x16 blocks, 4 kernels).

    timeout -k 10 300 python scripts/sample_area_each_timing.py --only a && \
    timeout -k 10 200 python scripts/sample_area_each_timing.py --only b        [--out profiles/render/sample_area_each_timing.txt]

Every GPU step under a time limit of its own: --only a writes the file, --only b appends to it.  (Without --only both run in
one process, with no limit but the caller's.)

(a) The fused call beside what the tree could do for the same result before it: every tap of every sample materialised as a
point on the device (blocks.area_taps_each's arithmetic in torch, the valid slots only, made once outside the windows),
smoe_sample_grad(want_values) on all of them, the masked sums per sample (index_add), the division and the lattice in torch.
Views, 1080x1920 samples each, taps = footprint_taps_each: a tilted view x_0 = 1080 + 0.7 (c_0 - 540) / s, x_1 = 0.7 c_1 / s,
s = 1 - 0.7 c_1 / 1920 (0.7 source pixels per sample at the left edge, 0.7 / s^2 = 7.8 along the tilt at the right edge, where
the view leaves the image), and a barrel-distortion map x = L / 2 + 2 (c - E / 2) (1 + 0.3 r^2), r the normalised radius;
each without blend and with blend = 2.
(b) Broadcast footprints beside smoe_sample_area on the three affine views of scripts/sample_area_timing.py: the price of
per-point generality (a product per tap and axis pair instead of a table read, F and taps loaded per point).
Method of scripts/sample_area_timing.py: after WARM launches, REPEATS windows between device events, the windows of the two ways
alternating; a window holds about 0.15 s of launches.  Reported: median and min..max microseconds per call, taps per second
from the median, and the ratio of the medians.  In the timed run the fused mean is compared with the other way's.  Every
measurement runs on the device or the script fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sample_area_timing import C, GRID, KPD, REPEATS, SHAPE, _measure, _stats  # noqa: E402


def _device_taps_each(torch, pts, foot, taps):
    """blocks.area_taps_each in torch on the device, the valid slots only: positions [T, d] and the owner of every tap [T]"""
    N, d = pts.shape
    n = taps.to(torch.int64)
    void = ((n < 1) | (n > 16)).any(dim=1) | (n.prod(dim=1) > 64) | ~torch.isfinite(foot).all(dim=2).all(dim=1)
    n = torch.where(void[:, None], torch.ones_like(n), n)
    t = torch.arange(64, device="cuda")[None, :]
    valid = (t < n.prod(dim=1)[:, None]) & ~void[:, None]
    owner, slot = valid.nonzero(as_tuple=True)
    r, nn, j = slot.clone(), n[owner], []
    for m in range(d - 1, -1, -1):
        j.insert(0, r % nn[:, m])
        r = r // nn[:, m]
    off = [(2 * j[m] + 1 - nn[:, m]).to(torch.float32) / (2 * nn[:, m]).to(torch.float32) for m in range(d)]
    cols = []
    for l in range(d):
        v = pts[owner, l]
        for m in range(d):
            v = v + foot[owner, l, m] * off[m]
        cols.append(v)
    return torch.stack(cols, dim=-1).contiguous(), owner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "sample_area_each_timing.txt"))
    ap.add_argument("--only", choices=["a", "b"], default=None, help="one comparison, appended to --out")
    args = ap.parse_args()
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    from steered_mixture_of_experts_amd.smoe import footprint_taps_each_torch, map_footprints_torch
    assert torch.cuda.is_available(), "sample_area_each_timing needs the GPU"
    os.environ.pop("SMOE_SAMPLE_RECORDS", None)
    B, K = int(np.prod(GRID)), int(np.prod(KPD))
    length = [g * n for g, n in zip(GRID, SHAPE)]
    p0 = blk.init_block_params(blk.synthetic_blocks(B, SHAPE, C, 7), KPD)
    eng = BlockEngine(EngineConfig(block_shape=SHAPE, channels=C, kernels=K, use_yuv=True, quantize_pis=True))
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")
    lines = []
    L, E = np.array(length, dtype=np.float64), (1080, 1920)

    def against_composition(name, pts, foot, beta):
        taps = footprint_taps_each_torch(foot)
        n = int(pts.shape[0])
        tap_dev, owner = _device_taps_each(torch, pts, foot, taps)
        nt = int(tap_dev.shape[0])
        img = torch.empty((n, C), dtype=torch.float32, device="cuda")
        jac = torch.empty((nt, 2, C), dtype=torch.float32, device="cuda")
        held = {}

        def fused():
            held["fused"] = eng.sample_area_each(dp, act, GRID, length, pts, foot, taps, blend=beta, out=img, want_mean=True, want_count=True)

        def composed():
            _, val, bk = eng.sample_grad(dp, act, GRID, length, tap_dev, blend=beta, out=jac, want_values=True, want_block=True)
            ins = bk >= 0
            cnt = torch.zeros((n,), dtype=torch.float32, device="cuda").index_add_(0, owner, ins.to(torch.float32))
            total = torch.zeros((n, C), dtype=torch.float32, device="cuda").index_add_(0, owner, val * ins[:, None])
            mean = torch.where(cnt[:, None] > 0, total / cnt.clamp(min=1)[:, None], torch.zeros_like(total))
            held["composed"] = (torch.floor(mean * 255.0 + 0.5) / 255.0, mean, cnt)

        ts = _measure({"sample_area_each": fused, "sample_grad_and_torch_mean": composed}, torch)
        tn = taps.to(torch.int64).prod(dim=1)
        rec = {"case": name, "samples": n, "taps": nt, "taps_per_sample_mean_max": [round(nt / n, 2), int(tn.max())],
               "tap_tuples": int(torch.unique(taps, dim=0).shape[0]), "blend": 0.0 if beta is None else beta,
               **{k: _stats(v, nt) for k, v in ts.items()}}
        rec["composition_over_fused_time"] = round(rec["sample_grad_and_torch_mean"]["us"] / rec["sample_area_each"]["us"], 3)
        fv, fm, fc = held["fused"]
        cv, cm, cc = held["composed"]
        rec["taps_inside_share"] = round(float(fc.to(torch.float32).sum()) / nt, 4)
        rec["max_abs_mean_difference"] = float((fm - cm).abs().max())
        rec["lattice_values_equal"] = round(float(((fv - cv).abs() < 1e-7).float().mean()), 6)
        assert torch.equal(fc.to(torch.float32), cc) and torch.isfinite(fm).all()
        assert rec["max_abs_mean_difference"] < 1e-5 and rec["lattice_values_equal"] > 0.999
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del img, jac, held, tap_dev, owner
        torch.cuda.empty_cache()

    def against_sample_area(name, A, size, taps, beta):
        F = np.asarray(A, dtype=np.float64)[:, :2].astype(np.float32)
        pts = torch.from_numpy(blk.warp_points(A, size).reshape(-1, 2)).cuda()
        n, nt = int(pts.shape[0]), int(np.prod(taps))
        foot = torch.from_numpy(F).cuda()[None].expand(n, 2, 2).contiguous()
        tp = torch.tensor(taps, dtype=torch.uint8, device="cuda")[None].expand(n, 2).contiguous()
        o1 = torch.empty((n, C), dtype=torch.float32, device="cuda")
        o2 = torch.empty((n, C), dtype=torch.float32, device="cuda")
        held = {}

        def one():
            held["one"] = eng.sample_area(dp, act, GRID, length, pts, F, taps, blend=beta, out=o1, want_mean=True, want_count=True)

        def each():
            held["each"] = eng.sample_area_each(dp, act, GRID, length, pts, foot, tp, blend=beta, out=o2, want_mean=True, want_count=True)

        ts = _measure({"sample_area": one, "sample_area_each": each}, torch)
        rec = {"case": name, "samples": n, "taps": "x".join(map(str, taps)), "blend": 0.0 if beta is None else beta,
               **{k: _stats(v, n * nt) for k, v in ts.items()}}
        rec["each_over_one_footprint_time"] = round(rec["sample_area_each"]["us"] / rec["sample_area"]["us"], 3)
        rec["bit_identical"] = all(bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(held["one"], held["each"]))
        assert rec["bit_identical"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if args.only in (None, "a"):
        H = np.array([[0.7, -0.7 / E[1] * L[0] / 2, -0.7 * E[0] / 2 + L[0] / 2], [0.0, 0.7, 0.0], [0.0, -0.7 / E[1], 1.0]])
        pts, foot, valid = blk.projective_points(H, E)
        assert valid.all()
        tilt = (torch.from_numpy(pts.reshape(-1, 2)).cuda(), torch.from_numpy(foot.reshape(-1, 2, 2)).cuda())
        c = np.stack(np.meshgrid(*[np.arange(e, dtype=np.float64) + 0.5 - e / 2 for e in E], indexing="ij"), axis=-1)
        r2 = (c ** 2).sum(axis=-1) / ((np.array(E) / 2) ** 2).sum()
        bar = torch.from_numpy((L / 2 + 2.0 * c * (1.0 + 0.3 * r2)[..., None]).astype(np.float32)).cuda()
        barrel = (bar.reshape(-1, 2).contiguous(), map_footprints_torch(bar).reshape(-1, 2, 2).contiguous())
        for beta in (None, 2.0):
            against_composition("tilted view 1080x1920, 0.7 to 7.8 px per sample", tilt[0], tilt[1], beta)
        for beta in (None, 2.0):
            against_composition("barrel map 1080x1920, k = 0.3", barrel[0], barrel[1], beta)
    if args.only in (None, "b"):
        c17, s17 = 3 * np.cos(np.deg2rad(17.0)), 3 * np.sin(np.deg2rad(17.0))
        M = np.array([[c17, -s17], [s17, c17]])
        rot = np.concatenate([M, (L / 2 - M @ (np.array([720.0, 1280.0]) / 2))[:, None]], axis=1)
        for beta in (None, 2.0):
            against_sample_area("1/8 thumbnail", [[8, 0, 0], [0, 8, 0]], (270, 480), (8, 8), beta)
        for beta in (None, 2.0):
            against_sample_area("1/2 view", [[2, 0, 0], [0, 2, 0]], (1080, 1920), (2, 2), beta)
        for beta in (None, 2.0):
            against_sample_area("1/3 view rotated by 17 degrees", rot, (720, 1280), (3, 3), beta)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = ("scripts/sample_area_each_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_sample_area_each (values, mean, count) on the "
            "cfg4-sized model (2160x3840 RGB, 16x16 blocks, 4 kernels); (a) beside smoe_sample_grad(want_values) on the materialised taps "
            "plus the masked mean and the lattice in torch, (b) with broadcast footprints beside smoe_sample_area.\nus: median per call "
            "over %d alternating windows (min..max); Gtaps_per_s: taps per second from the median; the ratios are ratios of the medians; "
            "the tap list of the composition is made outside its windows.\n" % REPEATS)
    fresh = args.only in (None, "a")                     # (b alone appends to what a wrote)
    with open(args.out, "w" if fresh else "a") as f:
        if fresh:
            f.write(head)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
