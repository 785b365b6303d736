"""Decoder timing (smoe_render) against the evaluation pass (smoe_forward, reconstruction only) on the same blocks.

    python scripts/render_timing.py            # every case, each in a child process of its own under a time limit;
                                               # stops at the first failure
    python scripts/render_timing.py --case gray65536

Per case and (samples per block, dtype): REPEATS windows of LAUNCHES launches between device events, the forward windows
alternating with the render windows; mean and min..max over the windows for both.  Written bytes = the image the launch
stores.  The end-to-end case times get_reconstruction() (evaluation pass + device-to-host copy + numpy stitch) against
Smoe.render(scale=1, to_host=False) with a host clock around a synchronise.

    python scripts/render_timing.py --shared   # the shared-kernel mode (smoe_shared_render against smoe_shared_forward), same
                                               # method; profiles/render/shared_render_timing.txt holds its output"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAUNCHES, REPEATS, WARM = 100, 5, 20
# name: block shape, C, kernels per dim, block grid, image shape in pixels, sample grids
CASES = {
    "gray65536": ((16, 16), 1, [2, 2], (256, 256), (4096, 4096), [(16, 16), (32, 32), (48, 48)]),
    "cfg4": ((16, 16), 3, [2, 2], (135, 240), (2160, 3840), [(16, 16), (32, 32), (48, 48)]),
    "cfg3": ((32, 32), 3, [2, 4], (34, 60), (1080, 1920), [(32, 32), (64, 64), (96, 96)]),
    "cfg5": ((16, 16, 4), 3, [2, 2, 1], (34, 60, 4), (544, 960, 16), [(16, 16, 4), (32, 32, 8), (48, 48, 12), (16, 16, 7)]),
}
LIMITS = {"gray65536": 240, "cfg4": 300, "cfg3": 200, "cfg5": 300, "end_to_end": 300}


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
    shape, C, kpd, grid, image, grids = CASES[name]
    B, K, N = int(np.prod(grid)), int(np.prod(kpd)), int(np.prod(shape))
    blocks = blk.synthetic_blocks(B, shape, C, 7)
    p0 = blk.init_block_params(blocks, kpd)
    eng = BlockEngine(EngineConfig(block_shape=shape, channels=C, kernels=K, use_yuv=(C == 3), quantize_pis=True))
    T = torch.from_numpy(blk.to_planar(blocks)).cuda()
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    act = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device="cuda")

    def fwd():
        eng.forward(T, dp, act, want_recon=True, update_active=False)

    for m in grids:
        extent = [image[l] * m[l] // shape[l] for l in range(len(shape))]
        axes = [torch.from_numpy(blk.render_axis(shape[l], m[l])).cuda() for l in range(len(shape))]
        for dtype, dname, esz in ((torch.float32, "f32", 4), (torch.uint8, "u8", 1)):
            out = torch.empty(tuple(extent) + (C,), dtype=dtype, device="cuda")

            def ren():
                eng.render(dp, act, axes, grid, extent, out=out, dtype=dtype)

            for _ in range(WARM):
                fwd()
                ren()
            torch.cuda.synchronize()
            tf, tr = [], []
            for _ in range(REPEATS):
                tf.append(_window(fwd, torch))
                tr.append(_window(ren, torch))
            samples = int(np.prod(extent))
            byt = samples * C * esz
            print(json.dumps({
                "case": name, "blocks": B, "samples_per_block": list(m), "extent": extent, "dtype": dname,
                "forward_recon_us": round(float(np.mean(tf)), 2), "forward_min_max_us": [round(min(tf), 2), round(max(tf), 2)],
                "forward_written_GBps": round(B * N * C * 4 / np.mean(tf) / 1e3, 1),
                "render_us": round(float(np.mean(tr)), 2), "render_min_max_us": [round(min(tr), 2), round(max(tr), 2)],
                "render_written_GBps": round(byt / np.mean(tr) / 1e3, 1),
                "render_Gsamples_per_s": round(samples / np.mean(tr) / 1e3, 2)}), flush=True)
    eng.close()


def run_end_to_end():
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.smoe import Smoe
    shape, C, kpd, grid, image, _ = CASES["cfg4"]
    b = blk.synthetic_blocks(int(np.prod(grid)), shape, C, 7)
    img = blk.blocks_to_image(b, image, shape)
    s = Smoe(img, train_inverse_cov=False, kernels_per_dim=kpd, batch_size=list(shape), use_determinant=True, quantize_pis=True)
    ta, tb = [], []
    for i in range(REPEATS + 1):
        s.valid = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = s.get_reconstruction()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = s.render(scale=1, to_host=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i:                                             # the first round warms both paths
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
    same = bool(np.array_equal(out.cpu().numpy(), rec))
    print(json.dumps({"case": "end_to_end cfg4", "get_reconstruction_ms": round(float(np.mean(ta)), 3),
                      "get_reconstruction_min_max_ms": [round(min(ta), 3), round(max(ta), 3)],
                      "render_to_device_ms": round(float(np.mean(tb)), 3), "render_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
                      "ratio": round(float(np.mean(ta) / np.mean(tb)), 1), "identical": same}), flush=True)


# ---- shared-kernel mode: smoe_shared_render against smoe_shared_forward ------------------------------------------------
SHARED_LAUNCHES, SHARED_WARM, SHARED_FIT = {"shared512": 500, "shared2160": 20}, 3, 20       # launches per window
# name: image shape, batch shape, C, kernels per dim, scales
SHARED_CASES = {
    "shared512": ((512, 512), (32, 32), 1, [12, 12], [1, 2, 4]),            # profiles/r03/bench_shared_mode.json
    "shared2160": ((2160, 3840), (16, 16), 3, [48, 80], [1, 2, 4]),
}
SHARED_LIMITS = {"shared512": 240, "shared2160": 420, "shared_end_to_end": 240}


def _shared_window(fn, torch, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches          # us per launch


def _shared_image(shape, C):
    from steered_mixture_of_experts_amd import blocks as blk
    g = [-(-s // 16) for s in shape]
    b = blk.synthetic_blocks(int(np.prod(g)), (16, 16), C, 7)
    return np.ascontiguousarray(blk.blocks_to_image(b, tuple(gi * 16 for gi in g), (16, 16))[:shape[0], :shape[1]])


def run_shared_case(name):
    import torch
    from steered_mixture_of_experts_amd import blocks as blk
    from steered_mixture_of_experts_amd.engine import SharedConfig, SharedEngine
    shape, bs, C, kpd, scales = SHARED_CASES[name]
    d = len(shape)
    img = _shared_image(shape, C)
    p0 = {k: v[0] for k, v in blk.init_block_params(img[None], kpd).items()}
    K = int(p0["pis"].shape[0])
    eng = SharedEngine(SharedConfig(image_shape=shape, batch_shape=bs, channels=C, kernels=K, use_yuv=(C == 3)))
    NB, Nb = eng.num_batches, eng.batch_pixels
    tb, _ = blk.image_to_blocks(img, bs)
    T = torch.from_numpy(blk.to_planar(tb)).cuda()
    dp = {k: torch.from_numpy(v).cuda() for k, v in p0.items()}
    lists = eng.new_lists()
    # the lists as they are after a short fit: evaluation (prunes), SHARED_FIT iterations, readmission, evaluation
    eng.forward(T, dp, lists, want_recon=False)
    eng.fit(T, dp, eng.new_adam_state(dp), lists, SHARED_FIT)
    eng.update_kernel_list(dp, lists)
    eng.forward(T, dp, lists, want_recon=False)
    torch.cuda.synchronize()
    words = lists.cpu().numpy().view(np.uint32)
    mean_len = float(np.mean([sum(bin(int(w)).count("1") for w in row) for row in words]))
    grid = [s // b for s, b in zip(shape, bs)]
    launches = SHARED_LAUNCHES[name]

    def fwd():
        eng.forward(T, dp, lists, want_recon=True, update_lists=False)

    def line(m, dtype, dname, esz, use_lists):
        extent = [g * v for g, v in zip(grid, m)]
        axes = [torch.from_numpy(blk.render_axis(shape[l], extent[l])).cuda() for l in range(d)]
        out = torch.empty(tuple(extent) + (C,), dtype=dtype, device="cuda")
        li = lists if use_lists else None

        def ren():
            eng.render(dp, li, axes, m, out=out, dtype=dtype)

        for _ in range(SHARED_WARM):
            fwd()
            ren()
        torch.cuda.synchronize()
        tf, tr = [], []
        for _ in range(REPEATS):
            n = max(5, launches // 25) if not use_lists else launches       # every kernel everywhere: long launches
            tf.append(_shared_window(fwd, torch, n))
            tr.append(_shared_window(ren, torch, n))
        samples = int(np.prod(extent))
        print(json.dumps({
            "case": name, "batches": NB, "kernels": K, "mean_list_length": round(mean_len, 1) if use_lists else K,
            "use_lists": use_lists, "samples_per_batch": list(m), "extent": extent, "dtype": dname,
            "forward_recon_us": round(float(np.mean(tf)), 2), "forward_min_max_us": [round(min(tf), 2), round(max(tf), 2)],
            "forward_written_GBps": round(NB * Nb * C * 4 / np.mean(tf) / 1e3, 1),
            "render_us": round(float(np.mean(tr)), 2), "render_min_max_us": [round(min(tr), 2), round(max(tr), 2)],
            "render_written_GBps": round(samples * C * esz / np.mean(tr) / 1e3, 1),
            "render_Gsamples_per_s": round(samples / np.mean(tr) / 1e3, 2),
            "render_ns_per_sample_and_listed_kernel": round(float(np.mean(tr)) * 1e3 / samples / (mean_len if use_lists else K), 4)}),
            flush=True)

    for sc in scales:
        m = [sc * b for b in bs]
        for dtype, dname, esz in ((torch.float32, "f32", 4), (torch.uint8, "u8", 1)):
            line(m, dtype, dname, esz, True)
    line(list(bs), torch.float32, "f32", 4, False)
    eng.close()


def run_shared_end_to_end():
    import torch
    from steered_mixture_of_experts_amd.smoe import Adam, SharedSmoe
    shape, bs, C, kpd, _ = SHARED_CASES["shared512"]
    s = SharedSmoe(_shared_image(shape, C), train_inverse_cov=False, kernels_per_dim=kpd, batch_size=list(bs), use_determinant=True)
    s.set_optimizer(Adam(1e-3), Adam(1e-5), Adam(1.0))
    s.train(SHARED_FIT, val_iter=SHARED_FIT)
    ta, tb = [], []
    for i in range(REPEATS + 1):
        s.valid = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = s.get_reconstruction()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = s.render(scale=1, to_host=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i:                                             # the first round warms both paths
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
    same = bool(np.array_equal(out.cpu().numpy(), rec))
    print(json.dumps({"case": "shared_end_to_end shared512", "get_reconstruction_ms": round(float(np.mean(ta)), 3),
                      "get_reconstruction_min_max_ms": [round(min(ta), 3), round(max(ta), 3)],
                      "render_to_device_ms": round(float(np.mean(tb)), 3), "render_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
                      "ratio": round(float(np.mean(ta) / np.mean(tb)), 1), "identical": same}), flush=True)


def _run_children(names, limits):
    for name in names:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], timeout=limits[name]).returncode
        if rc != 0:
            print(f"case {name} failed with exit status {rc}: stopping", flush=True)
            sys.exit(rc if rc > 0 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--shared", action="store_true", help="the shared-kernel mode cases instead of the block-mode ones")
    args = ap.parse_args()
    if args.case == "shared_end_to_end":
        return run_shared_end_to_end()
    if args.case in SHARED_CASES:
        return run_shared_case(args.case)
    if args.shared:
        return _run_children(list(SHARED_CASES) + ["shared_end_to_end"], SHARED_LIMITS)
    if args.case == "end_to_end":
        return run_end_to_end()
    if args.case:
        return run_case(args.case)
    for name in list(CASES) + ["end_to_end"]:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], timeout=LIMITS[name]).returncode
        if rc != 0:
            print(f"case {name} failed with exit status {rc}: stopping", flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
