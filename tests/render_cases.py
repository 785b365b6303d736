"""What the GPU suites of the three decoders (tests/test_gpu_render.py, test_gpu_render_blend.py, test_gpu_shared_render.py)
share: engines, inputs on the device, sample tables, guarded output buffers.  TEST INFRASTRUCTURE, never imported by the
product; imports torch only, no device is touched before a helper is called."""
import numpy as np
import torch

from oracle import smoe_oracle as o
from render_engine import place_blocks
from steered_mixture_of_experts_amd import blocks as blk
from steered_mixture_of_experts_amd.blocks import synthetic_blocks


def _lattice(precision=8):
    """(levels, influence threshold, half-width of the band around it) of a pixel lattice of ``precision`` bits: 255,
    0.5 / 256 and 1e-6 at 8 bits; the band keeps its share of the threshold (tests/step_parity.influence_threshold)"""
    return 2 ** precision - 1, 0.5 / 2 ** precision, 1e-6 * 2.0 ** (8 - precision)


def _engine(shape, C_, K, **kw):
    from steered_mixture_of_experts_amd.engine import BlockEngine, EngineConfig
    return BlockEngine(EngineConfig(block_shape=shape, channels=C_, kernels=K, **kw))


def _to_dev(p):
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in p.items()}


def _mask_to_bits(mask):
    """(n, K) bool -> (n, ceil(K / 32)) uint32 words, kernel k = bit k & 31 of word k >> 5"""
    n, K = mask.shape
    out = np.zeros((n, (K + 31) // 32), np.uint32)
    for k in range(K):
        out[:, k >> 5] |= (mask[:, k].astype(np.uint32) << np.uint32(k & 31))
    return out


def _bits(mask, words=False):
    """the kernel lists on the device as the entry points take them: int32 [n] (block mode: one word), or with ``words`` the
    [n, KW] bitmaps of shared mode"""
    w = _mask_to_bits(mask)
    assert words or w.shape[1] == 1
    return torch.from_numpy(np.ascontiguousarray(w if words else w[:, 0]).view(np.int32)).cuda()


def _setup(shape, C_, kpd, yuv, B, seed, **cfgkw):
    """parameters as test_forward_parity draws them (perturbed initialisation)"""
    K = int(np.prod(kpd))
    b = synthetic_blocks(B, shape, C_, seed)
    p = o.init_params(b, kpd)
    rng = np.random.default_rng(seed + 1)
    p["A_corr"] = (rng.normal(size=p["A_corr"].shape) * 1.5).astype(np.float32)
    p["A_diagonal"] = (p["A_diagonal"] + rng.normal(size=p["A_diagonal"].shape)).astype(np.float32)
    p["gamma_e"] = (rng.normal(size=p["gamma_e"].shape) * 0.1).astype(np.float32)
    p["musX"] = (p["musX"] + rng.normal(size=p["musX"].shape) * 0.05).astype(np.float32)
    p["pis"] = (p["pis"] * rng.uniform(0.5, 1.5, size=p["pis"].shape)).astype(np.float32)
    cfg = o.OracleConfig(block_shape=shape, channels=C_, kernels=K, use_yuv=yuv, **cfgkw)
    return cfg, p, b.reshape(B, -1, C_), K


def _axes(n, m):
    return [blk.render_axis(a, b) for a, b in zip(n, m)]


def _dev_axes(tabs):
    return [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in tabs]


def _owned(m, grid, extent, first, count):
    """bool [*extent]: positions of the blocks [first, first + count)"""
    own = np.zeros(tuple(extent) + (1,), dtype=bool)
    ones = np.ones((count, int(np.prod(m)), 1), dtype=bool)
    return place_blocks(ones, m, grid, extent, first, own)[..., 0]


def _guarded(shape, dtype, fill, guard=64, shift=0):
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard + 8,), fill, dtype=dtype, device="cuda")
    return buf, buf[guard + shift: guard + shift + n].view(*shape)


def _image(h, w, C_=1, seed=0):
    gh, gw = -(-h // 16), -(-w // 16)
    b = synthetic_blocks(gh * gw, (16, 16), C_, seed)
    return blk.blocks_to_image(b, (gh * 16, gw * 16), (16, 16))[:h, :w]
