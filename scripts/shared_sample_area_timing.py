"""Timing of the area-averaged decoder of whole-image models (smoe_shared_sample_area: SharedSmoe.eval_points_area,
eval_view(taps=...), eval_warp(taps=...)) on the two whole-image models of profiles/render/shared_sample_timing.txt, beside what
the tree could do for the same result before it: every tap materialised as a point, smoe_shared_sample_grad(want_values) on all
of them, the masked mean and the lattice in torch.

    python scripts/shared_sample_area_timing.py [--out profiles/render/shared_sample_area_timing.txt] [--cases shared512,shared2160]
                                                [--tile 512] [--append]

Per model (set up as scripts/shared_sample_timing.py does: lists after a 20-iteration fit): (a) a 1/8 thumbnail of the whole
image with 8x8 taps; (b) a 1/2 view with 2x2 taps; (c) a 1/3 view rotated by 17 degrees about the image centre with 3x3 taps
(its corners leave the image: their taps are left out of the mean).  Method of scripts/sample_area_timing.py: after WARM
launches, REPEATS windows between device events, the windows of the two ways alternating; reported are the median and min..max
microseconds per call, taps per second from the median and the time ratio composition / fused.  The tap list of the composition
is made once, outside its windows.  The timed composition sums the taps with torch's sum (the fastest way to write it; it
associates differently); the check of the timed run repeats the mean once in the stated order -- tap by tap -- and compares it
with the fused mean BIT FOR BIT, the counts exactly, and the lattice values.  batches_per_workgroup: the distinct batches among
the taps of the TILE / T consecutive points a workgroup takes (--tile: SSA_TILE of the library under test), mean and maximum:
what a workgroup walks.  Every measurement runs on the device or the script fails."""
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


def _visits(torch, bk, n, nt, tile):
    """distinct batches (>= 0) per workgroup of tile // nt points: (mean, max)"""
    P = tile // nt
    W = -(-n // P)
    b = torch.full((W * P * nt,), -1, dtype=torch.int32, device="cuda")
    b[:n * nt] = bk.reshape(-1)
    s, _ = torch.sort(b.reshape(W, P * nt), dim=1)
    new = torch.cat([s[:, :1] >= 0, (s[:, 1:] != s[:, :-1]) & (s[:, 1:] >= 0)], dim=1).sum(dim=1).to(torch.float32)
    return round(float(new.mean()), 2), int(new.max())


def run_case(name, tile, emit):
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
    head = {"model": name, "SSA_TILE": tile, "batches": eng.num_batches, "kernels": K, "mean_list_length": round(mean_len, 1)}

    def case(label, A, size, taps):
        F = np.asarray(A, dtype=np.float64)[:, :2].astype(np.float32)
        host = blk.warp_points(A, size).reshape(-1, 2)
        pts = torch.from_numpy(host).cuda()
        n, nt = int(pts.shape[0]), int(np.prod(taps))
        tap_dev = torch.from_numpy(blk.area_taps(host, F, taps).reshape(-1, 2)).cuda()
        out = torch.empty((n, C), dtype=torch.float32, device="cuda")
        jac = torch.empty((n * nt, 2, C), dtype=torch.float32, device="cuda")
        held = {}

        def fused():
            held["fused"] = eng.sample_area(dp, lists, pts, F, taps, out=out, want_mean=True, want_count=True)

        def composed():
            _, val, bk = eng.sample_grad(dp, lists, tap_dev, out=jac, want_values=True, want_batch=True)
            ins = (bk >= 0).reshape(n, nt)
            cnt = ins.sum(dim=1)
            total = (val.reshape(n, nt, C) * ins[:, :, None]).sum(dim=1)
            mean = torch.where(cnt[:, None] > 0, total / cnt.clamp(min=1).to(torch.float32)[:, None], torch.zeros_like(total))
            held["composed"] = (torch.floor(mean * 255.0 + 0.5) / 255.0, mean, cnt, val, bk)

        ts = _measure({"shared_sample_area": fused, "shared_sample_grad_and_torch_mean": composed}, torch)
        rec = dict(head, case=label, samples=n, taps="x".join(map(str, taps)), **{k: _stats(v, n * nt) for k, v in ts.items()})
        rec["composition_over_fused_time"] = round(rec["shared_sample_grad_and_torch_mean"]["us"] / rec["shared_sample_area"]["us"], 3)
        fv, fm, fc = held["fused"]
        cv, cm, cc, val, bk = held["composed"]
        # the mean once more in the stated order, tap by tap: bit for bit the fused one
        V, ins = val.reshape(n, nt, C), (bk >= 0).reshape(n, nt)
        acc = torch.zeros((n, C), dtype=torch.float32, device="cuda")
        for t in range(nt):
            acc = torch.where(ins[:, t, None], acc + V[:, t], acc)
        ordered = torch.where(cc[:, None] > 0, acc / cc.clamp(min=1).to(torch.float32)[:, None], torch.zeros_like(acc))
        rec["taps_inside_share"] = round(float(fc.to(torch.float32).mean()) / nt, 4)
        rec["counts_equal"] = bool(torch.equal(fc.to(torch.int64), cc))
        rec["mean_bit_identical_to_ordered_composition"] = bool(torch.equal(fm.view(torch.int32), ordered.view(torch.int32)))
        rec["max_abs_difference_to_torch_sum_mean"] = float((fm - cm).abs().max())
        rec["lattice_values_equal_share"] = round(float(((fv - cv).abs() < 1e-7).float().mean()), 6)
        rec["batches_per_workgroup_mean_max"] = _visits(torch, bk, n, nt, tile)
        assert rec["counts_equal"] and rec["mean_bit_identical_to_ordered_composition"] and torch.isfinite(fm).all()
        emit(rec)
        del out, jac, held, tap_dev, V, acc
        torch.cuda.empty_cache()

    L = np.array(shape, dtype=np.float64)
    case("1/8 thumbnail", [[8, 0, 0], [0, 8, 0]], (shape[0] // 8, shape[1] // 8), (8, 8))
    case("1/2 view", [[2, 0, 0], [0, 2, 0]], (shape[0] // 2, shape[1] // 2), (2, 2))
    c17, s17 = 3 * np.cos(np.deg2rad(17.0)), 3 * np.sin(np.deg2rad(17.0))
    M = np.array([[c17, -s17], [s17, c17]])
    E = (shape[0] // 3, shape[1] // 3)
    rot = np.concatenate([M, (L / 2 - M @ (np.array(E, dtype=np.float64) / 2))[:, None]], axis=1)
    case("1/3 view rotated by 17 degrees", rot, E, (3, 3))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "shared_sample_area_timing.txt"))
    ap.add_argument("--cases", default="shared512,shared2160")
    ap.add_argument("--tile", type=int, default=512, help="SSA_TILE of the library under test (labels the lines)")
    ap.add_argument("--append", action="store_true", help="add the lines to an existing file (a second build)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "shared_sample_area_timing needs the GPU"
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for name in args.cases.split(","):
        run_case(name, args.tile, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        if not args.append:
            f.write("scripts/shared_sample_area_timing.py on " + torch.cuda.get_device_name(0) + ": smoe_shared_sample_area (values, "
                    "mean, count) beside smoe_shared_sample_grad(want_values) on the materialised taps plus the masked mean and the "
                    "lattice in torch, the two models of shared_sample_timing.txt (lists after a %d-iteration fit).\nus: median per call "
                    "over %d alternating windows (min..max); Gtaps_per_s: taps per second from the median; composition_over_fused_time: "
                    "ratio of the medians; the tap list of the composition is made outside its windows; SSA_TILE: taps per workgroup of "
                    "the build that was timed; batches_per_workgroup_mean_max: distinct batches among a workgroup's taps.\n"
                    % (FIT, REPEATS))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
