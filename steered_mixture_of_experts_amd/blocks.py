"""Host-side block plumbing: image <-> independent blocks, the reference's initialisers,
deterministic synthetic data.  NumPy only; runs once per fit (not the hot path).

Block order is the reference's ``sliding_window`` order (smoe.py:18-35): y outer, x inner,
t innermost.  Every block is its own [0,1]^d domain (smoe.py:2412), i.e. ``blocks[b]`` is what
``Smoe(block_b, ...)`` would see.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Dict, List, Sequence, Tuple

import numpy as np


# ------------------------------------------------------------------------------------
# tiling
# ------------------------------------------------------------------------------------
def padded_shape(domain_shape: Sequence[int], block_shape: Sequence[int]) -> Tuple[int, ...]:
    return tuple(int(-(-s // b) * b) for s, b in zip(domain_shape, block_shape))


def grid_shape(domain_shape: Sequence[int], block_shape: Sequence[int]) -> Tuple[int, ...]:
    return tuple(int(-(-s // b)) for s, b in zip(domain_shape, block_shape))


def image_to_blocks(image: np.ndarray, block_shape: Sequence[int]):
    """(H,W[,T],C) -> blocks (B, *block_shape, C) in sliding_window order, plus a validity
    mask (B, N) that is 0 on padding.  The reference raises when the image is not a multiple
    of the block (smoe.py:239-241); here the image is edge-replicated up to the next multiple
    and padded pixels get loss weight 0 (the graph's per-pixel ``loss_weights``, smoe.py:550,932)."""
    d = image.ndim - 1
    bs = tuple(int(b) for b in block_shape)
    assert len(bs) == d
    dom = image.shape[:d]
    pad = padded_shape(dom, bs)
    if pad != tuple(dom):
        widths = [(0, p - s) for s, p in zip(dom, pad)] + [(0, 0)]
        img = np.pad(image, widths, mode="edge")
        valid = np.pad(np.ones(dom, dtype=np.float32), widths[:-1], mode="constant")
    else:
        img = image
        valid = np.ones(dom, dtype=np.float32)
    g = grid_shape(dom, bs)
    C = image.shape[-1]
    # (g0,b0,g1,b1[,g2,b2],C) -> (g0,g1[,g2],b0,b1[,b2],C)
    split = []
    for gi, bi in zip(g, bs):
        split += [gi, bi]
    perm = list(range(0, 2 * d, 2)) + list(range(1, 2 * d, 2))
    blocks = img.reshape(split + [C]).transpose(perm + [2 * d]).reshape((-1,) + bs + (C,))
    vblk = valid.reshape(split).transpose(perm).reshape(-1, int(np.prod(bs)))
    return np.ascontiguousarray(blocks), np.ascontiguousarray(vblk)


def blocks_to_image(blocks: np.ndarray, domain_shape: Sequence[int], block_shape: Sequence[int]) -> np.ndarray:
    """Inverse of image_to_blocks (crops the padding): (B, *block_shape, X) -> (*domain_shape, X).
    Mirrors the stitch of smoe.py:1719-1744."""
    d = len(block_shape)
    bs = tuple(int(b) for b in block_shape)
    g = grid_shape(domain_shape, bs)
    tail = blocks.shape[1 + d:]
    arr = blocks.reshape(tuple(g) + bs + tail)
    perm = []
    for i in range(d):
        perm += [i, d + i]
    perm += list(range(2 * d, 2 * d + len(tail)))
    arr = arr.transpose(perm).reshape(tuple(gi * bi for gi, bi in zip(g, bs)) + tail)
    sl = tuple(slice(0, s) for s in domain_shape)
    return arr[sl]


def render_axis(n: int, m: int) -> np.ndarray:
    """Coordinates (block units, float32) of ``m`` render samples along a block axis fitted on ``n`` pixels -- the one
    definition of the mapping behind ``Smoe.render``.  ``m == n``: the training lattice ``linspace(0, 1, n)`` itself;
    otherwise the centres of ``m`` equal cells over the block's pixel footprint, ``((j + 0.5) n / m - 0.5) / (n - 1)``:
    an output pixel of a 2x image sits where a 2x finer sensor would have it, and the first / last samples overhang the
    lattice by less than half a source pixel.  Computed in float64, rounded once."""
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError("render_axis: n and m must be >= 1")
    if n == 1:
        return np.zeros((m,), dtype=np.float32)
    if m == n:
        return np.linspace(0, 1, n).astype(np.float32)
    j = np.arange(m, dtype=np.float64)
    return (((j + 0.5) * n / m - 0.5) / (n - 1)).astype(np.float32)


def _round_once_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the exact ``x`` (ties to even): float64 first, then repaired where that second rounding
    starts from a float64 that sits exactly half way between two float32 while ``x`` itself does not."""
    d = float(x)
    r = np.float32(d)
    if float(r) != d:
        other = np.nextafter(r, np.float32(np.inf) if d > float(r) else np.float32(-np.inf))
        mid = (Fraction(float(r)) + Fraction(float(other))) / 2
        if Fraction(d) == mid and x != mid:
            r = other if (x > mid) == (float(other) > float(r)) else r
    return r


def view_axis(n: int, grid_l: int, length_l, lo, hi, E: int):
    """One axis of a viewport (``Smoe.render_view``, include/smoe_hip.h: smoe_render_view): ``E`` samples over the window
    ``[lo, hi)`` of an axis of ``length_l`` source pixels cut into ``grid_l`` blocks of ``n`` pixels.  Pixel-footprint
    convention of ``render_axis``: source pixel ``q`` covers ``[q, q + 1)``, ``0 <= lo < hi <= length_l``.  Sample ``i``
    sits at ``x_i = lo + (i + 0.5)(hi - lo) / E``, in block ``g = min(floor(x_i / n), grid_l - 1)``, at the block-unit
    coordinate ``(x_i - g n - 0.5) / (n - 1)`` (0 for ``n == 1``), computed exactly and rounded to float32 once.  Where a
    block's run coincides with ``render_axis(n, m)`` for an integer ``m`` (the pitch is ``n / m`` and the run's first
    sample is one of that table's) the values are THAT table's, so an aligned view is bit-identical to ``render``.
    Returns ``(first, blocks, start, coords)``: the first block of the view, the number of blocks it spans,
    ``start`` int32 ``[blocks + 1]`` (samples ``[start[j], start[j + 1])`` lie in block ``first + j``; runs may be empty)
    and ``coords`` float32 ``[E]``."""
    n, grid_l, E = int(n), int(grid_l), int(E)
    if n < 1 or grid_l < 1:
        raise ValueError("view_axis: n and grid_l must be >= 1")
    if E < 1 or E > 2 ** 31 - 1:
        raise ValueError("view_axis: E must be 1 .. 2^31 - 1")
    lo, hi, length = float(lo), float(hi), float(length_l)
    if not (0.0 <= lo < hi <= length) or length > grid_l * n:
        raise ValueError(f"view_axis: the window must satisfy 0 <= lo < hi <= length ({lo}, {hi}, {length})")
    flo, pitch = Fraction(lo), (Fraction(hi) - Fraction(lo)) / E
    # x_i = (P + (2 i + 1) Q) / R in integers: no fraction is reduced per sample
    half = pitch / 2
    R = math.lcm(flo.denominator, half.denominator)
    P, Q = flo.numerator * (R // flo.denominator), half.numerator * (R // half.denominator)
    nums = [P + (2 * i + 1) * Q for i in range(E)]
    gs = np.fromiter((min(v // (R * n), grid_l - 1) for v in nums), dtype=np.int64, count=E)
    first, blocks = int(gs[0]), int(gs[-1] - gs[0] + 1)
    start = np.searchsorted(gs, first + np.arange(blocks + 1), side="left").astype(np.int32)
    coords = np.zeros((E,), dtype=np.float32)
    if n == 1:
        return first, blocks, start, coords
    m = Fraction(n) / pitch
    table = render_axis(n, int(m)) if m.denominator == 1 else None
    for j in range(blocks):
        a, b = int(start[j]), int(start[j + 1])
        if a == b:
            continue
        g = first + j
        if table is not None:
            j0 = (Fraction(nums[a], R) - g * n) / pitch - Fraction(1, 2)
            if j0.denominator == 1 and 0 <= j0 and int(j0) + (b - a) <= len(table):
                coords[a:b] = table[int(j0):int(j0) + (b - a)]
                continue
        for i in range(a, b):
            coords[i] = _round_once_f32((Fraction(nums[i], R) - g * n - Fraction(1, 2)) / (n - 1))
    return first, blocks, start, coords


def view_positions(lo, hi, E: int) -> np.ndarray:
    """The sample positions of one axis of a viewport in source pixels, as ``view_axis`` places them: ``x_i = lo + (i + 0.5)
    (hi - lo) / E``, computed exactly (``lo`` and ``hi`` are taken as the float64 they are) and rounded to float32 once.
    Returns float32 ``[E]`` -- the cell centres ``Smoe.render_view(taps=...)`` hands to ``sample_area``."""
    E = int(E)
    if E < 1:
        raise ValueError("view_positions: E must be >= 1")
    flo, half = Fraction(float(lo)), (Fraction(float(hi)) - Fraction(float(lo))) / (2 * E)
    return np.array([_round_once_f32(flo + (2 * i + 1) * half) for i in range(E)], dtype=np.float32)


def point_blocks(points, block_shape: Sequence[int], grid: Sequence[int], length: Sequence[int]):
    """Where arbitrary positions fall (``Smoe.sample``, include/smoe_hip.h: smoe_sample) -- the one host statement of the
    mapping, in float32 throughout, as the kernel computes it.  ``points`` ``[..., d]`` in source pixels, axis order of the
    image; pixel ``q`` covers ``[q, q + 1)``; ``length[l]`` the true extent (``1 <= length[l] <= grid[l] * n_l``).  A point is
    outside if on any axis ``x`` is NaN, ``x < 0`` or ``x >= length[l]``.  Per axis the block is the integer ``g`` with
    ``g n <= x < (g + 1) n`` exactly (``floor(x / n)`` corrected by +-1 against the products, which are exact in float32 for
    ``grid[l] * n <= 2^24``), and the block-unit coordinate ``u = ((x - g n) - 0.5) / (n - 1)`` (0 for ``n == 1``): an exact
    subtraction, one rounded subtraction, one rounded division.  Returns ``(inside [...] bool, block [..., d] int64 (0 where
    outside), u [..., d] float32 (0 where outside))``."""
    pts = np.asarray(points, dtype=np.float32)
    d = len(block_shape)
    if pts.ndim < 1 or pts.shape[-1] != d or len(grid) != d or len(length) != d:
        raise ValueError(f"point_blocks: points need a trailing axis of {d}, grid and length {d} entries")
    for n, g, ln in zip(block_shape, grid, length):
        if int(n) < 1 or int(g) < 1 or not (1 <= int(ln) <= int(g) * int(n)) or int(g) * int(n) > 2 ** 24:
            raise ValueError("point_blocks: need n, grid >= 1, 1 <= length <= grid * n <= 2^24")
    inside = np.ones(pts.shape[:-1], dtype=bool)
    block = np.zeros(pts.shape, dtype=np.int64)
    u = np.zeros(pts.shape, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for l in range(d):
            inside &= (pts[..., l] >= np.float32(0)) & (pts[..., l] < np.float32(int(length[l])))
        for l in range(d):
            n = int(block_shape[l])
            x = np.where(inside, pts[..., l], np.float32(0)).astype(np.float32)
            g = np.floor(x / np.float32(n)).astype(np.int64)
            g = g - ((g * n).astype(np.float32) > x)
            g = g + (((g + 1) * n).astype(np.float32) <= x)
            t = x - (g * n).astype(np.float32)
            block[..., l] = g
            if n > 1:
                u[..., l] = np.where(inside, (t - np.float32(0.5)) / np.float32(n - 1), np.float32(0))
    return inside, block, u


def warp_points(matrix, size: Sequence[int]) -> np.ndarray:
    """The source positions of an affine view (``Smoe.render_warp``): output index ``i`` has its cell centre at ``i + 0.5`` and
    its source position is ``x = M (i + 0.5) + t`` for ``matrix = [M | t]`` of shape ``[d, d + 1]``, in source pixels
    (``point_blocks``' convention).  Computed in float64, rounded to float32 once.  Returns ``[*size, d]``."""
    A = np.asarray(matrix, dtype=np.float64)
    size = [int(v) for v in np.atleast_1d(size)]
    d = len(size)
    if A.shape != (d, d + 1) or not np.isfinite(A).all():
        raise ValueError(f"warp_points: matrix must be a finite [{d}, {d + 1}] array [M | t]")
    if min(size) < 1:
        raise ValueError("warp_points: size needs entries >= 1")
    idx = np.stack(np.meshgrid(*[np.arange(e, dtype=np.float64) + 0.5 for e in size], indexing="ij"), axis=-1)
    return (idx @ A[:, :d].T + A[:, d]).astype(np.float32)


AREA_AXIS_TAPS = 16     # taps per view axis of an area-averaged sample, at most (include/smoe_hip.h: smoe_sample_area)
AREA_TAPS = 64          # taps per sample, at most


def area_args(footprint, taps, d: int):
    """``footprint`` as float32 ``[d, d]`` and ``taps`` as ``d`` ints, checked as smoe_sample_area checks them."""
    F = np.asarray(footprint, dtype=np.float32)
    if F.shape != (d, d) or not np.isfinite(F).all():
        raise ValueError(f"footprint must be a finite [{d}, {d}] array")
    tp = [int(v) for v in np.atleast_1d(taps)]
    tp = tp * d if len(tp) == 1 else tp
    if len(tp) != d or min(tp) < 1 or max(tp) > AREA_AXIS_TAPS:
        raise ValueError(f"taps needs one value or {d}, each 1 .. {AREA_AXIS_TAPS}")
    if int(np.prod(tp)) > AREA_TAPS:
        raise ValueError(f"taps must not multiply to more than {AREA_TAPS}")
    return F, tp


def area_taps(points, footprint, taps) -> np.ndarray:
    """The tap positions of area-averaged samples (``Smoe.sample_area``, include/smoe_hip.h: smoe_sample_area) -- the one host
    statement of the arithmetic, in float32 throughout, as the kernel computes it.  ``points`` ``[N, d]``: the cell centres in
    source pixels; ``footprint`` ``[d, d]``: column ``m`` is the edge vector of an output cell along view axis ``m``;
    ``taps``: the taps per view axis (1 .. 16, product at most 64).  Tap ``j`` (row-major, last axis fastest) has the offset
    ``o_m = float32(2 j_m + 1 - taps[m]) / float32(2 taps[m])`` and the position ``t_l = x_l``, then for ``m = 0 .. d-1``:
    ``t_l = t_l + (F[l][m] * o_m)``, the product and the sum rounded separately.  Returns float32 ``[N, T, d]``."""
    pts = np.asarray(points, dtype=np.float32)
    if pts.ndim != 2:
        raise ValueError("area_taps: points must be [N, d]")
    d = pts.shape[1]
    F, tp = area_args(footprint, taps, d)
    off = [(np.arange(n, dtype=np.int64) * 2 + 1 - n).astype(np.float32) / np.float32(2 * n) for n in tp]
    jj = np.stack(np.meshgrid(*[np.arange(n) for n in tp], indexing="ij"), axis=-1).reshape(-1, d)       # [T, d] row-major
    out = np.empty((pts.shape[0], jj.shape[0], d), dtype=np.float32)
    for l in range(d):
        t = np.repeat(pts[:, l:l + 1], jj.shape[0], axis=1)
        for m in range(d):
            t = (t + (F[l, m] * off[m][jj[:, m]]).astype(np.float32)[None, :]).astype(np.float32)
        out[:, :, l] = t
    return out


def footprint_taps(footprint):
    """``taps="auto"`` of ``Smoe.sample_area``: one tap per source pixel the cell covers along each view axis,
    ``n_m = clamp(ceil(max_l |F[l][m]|), 1, 16)``, then the largest entry (the first of equals) is decremented until the
    product is at most 64.  Returns a tuple of ints."""
    F = np.asarray(footprint, dtype=np.float64)
    if F.ndim != 2 or F.shape[0] != F.shape[1] or not np.isfinite(F).all():
        raise ValueError("footprint_taps: footprint must be a finite [d, d] array")
    tp = [int(min(max(math.ceil(float(np.abs(F[:, m]).max())), 1), AREA_AXIS_TAPS)) for m in range(F.shape[1])]
    while int(np.prod(tp)) > AREA_TAPS:
        tp[int(np.argmax(tp))] -= 1
    return tuple(tp)


def area_void_each(footprints, taps) -> np.ndarray:
    """The void rule of smoe_sample_area_each (include/smoe_hip.h) for ``footprints`` ``[N, d, d]`` and ``taps`` ``[N, d]``:
    a point is void if a tap count is outside 1 .. 16, if the counts multiply to more than 64 or if an entry of its footprint
    is not finite.  Returns bool ``[N]``."""
    F = np.asarray(footprints, dtype=np.float32)
    tp = np.asarray(taps).astype(np.int64)
    return (tp < 1).any(axis=1) | (tp > AREA_AXIS_TAPS).any(axis=1) | (np.prod(np.clip(tp, 0, 255), axis=1) > AREA_TAPS) \
        | ~np.isfinite(F).all(axis=(1, 2))


def area_taps_each(points, footprints, taps):
    """The tap positions of area-averaged samples with a footprint of their own per point (``Smoe.sample_area_each``,
    include/smoe_hip.h: smoe_sample_area_each) -- the one host statement of the arithmetic: ``area_taps`` per point, in float32
    throughout.  ``points`` ``[N, d]``, ``footprints`` ``[N, d, d]``, ``taps`` ``[N, d]`` integers.  Slot ``t`` of point ``i``
    is its tap with the row-major index ``t`` under ITS counts (last axis fastest): offset ``o_m = float32(2 j_m + 1 - n_m) /
    float32(2 n_m)``, position ``t_l = x_l``, then for ``m = 0 .. d-1`` ``t_l = t_l + (F[l][m] * o_m)``, product and sum rounded
    separately.  Returns ``(positions float32 [N, 64, d], valid bool [N, 64])``: a slot past ``prod(taps[i])`` and every slot
    of a void point (``area_void_each``) is not valid and holds NaN."""
    pts = np.asarray(points, dtype=np.float32)
    if pts.ndim != 2:
        raise ValueError("area_taps_each: points must be [N, d]")
    N, d = pts.shape
    F = np.asarray(footprints, dtype=np.float32)
    tp = np.asarray(taps)
    if F.shape != (N, d, d) or tp.shape != (N, d) or tp.dtype.kind not in "iu":
        raise ValueError(f"area_taps_each: footprints must be [{N}, {d}, {d}] and taps integers [{N}, {d}]")
    void = area_void_each(F, tp)
    n = np.where(void[:, None], 1, tp.astype(np.int64))                                  # [N, d]
    t = np.arange(AREA_TAPS, dtype=np.int64)[None, :]                                    # [1, 64]
    valid = (t < np.prod(n, axis=1)[:, None]) & ~void[:, None]
    j = np.empty((N, AREA_TAPS, d), dtype=np.int64)
    r = np.broadcast_to(t, (N, AREA_TAPS)).copy()
    for m in range(d - 1, -1, -1):
        j[:, :, m] = r % n[:, None, m]
        r //= n[:, None, m]
    off = (2 * j + 1 - n[:, None, :]).astype(np.float32) / (2 * n[:, None, :]).astype(np.float32)      # [N, 64, d]
    out = np.empty((N, AREA_TAPS, d), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(d):
            v = np.repeat(pts[:, l:l + 1], AREA_TAPS, axis=1)
            for m in range(d):
                v = (v + (F[:, None, l, m] * off[:, :, m]).astype(np.float32)).astype(np.float32)
            out[:, :, l] = v
    out[~valid] = np.float32("nan")
    return out, valid


def footprint_taps_each(footprints) -> np.ndarray:
    """``taps="auto"`` of ``Smoe.sample_area_each``: ``footprint_taps``' rule per point, evaluated on the float32 entries --
    ``n_m = clamp(ceil(max_l |F[l][m]|), 1, 16)``, then the largest entry (the first of equals) is decremented until the
    product is at most 64.  A footprint with a non-finite entry gets taps 0, which marks the point void.  ``footprints``
    ``[N, d, d]``; returns uint8 ``[N, d]``."""
    F = np.asarray(footprints, dtype=np.float32)
    if F.ndim != 3 or F.shape[1] != F.shape[2]:
        raise ValueError("footprint_taps_each: footprints must be [N, d, d]")
    fin = np.isfinite(F).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        tp = np.clip(np.ceil(np.abs(np.where(fin[:, None, None], F, np.float32(0))).max(axis=1)), 1, AREA_AXIS_TAPS).astype(np.int64)
    rows = np.arange(F.shape[0])
    while True:
        over = np.prod(tp, axis=1) > AREA_TAPS
        if not over.any():
            break
        tp[rows[over], np.argmax(tp[over], axis=1)] -= 1
    tp[~fin] = 0
    return tp.astype(np.uint8)


def projective_points(H, size: Sequence[int]):
    """The source positions and footprints of a projective view (``Smoe.render_projective``): ``H`` ``[d + 1, d + 1]`` maps the
    cell centre ``c = i + 0.5`` of output index ``i`` to ``x = (H[:d, :d] c + H[:d, d]) / s`` with ``s = H[d, :d] . c + H[d, d]``,
    in source pixels; the footprint is the analytic Jacobian ``J[l][m] = (H[l][m] - x_l H[d][m]) / s``.  Computed in float64,
    rounded to float32 once.  Where ``s <= 0`` or ``s`` is not finite the sample is behind the horizon: ``valid`` False, the
    point NaN, the footprint 0.  With the last row ``(0, .., 0, 1)`` the points are ``warp_points([M | t], size)`` and every
    footprint is ``float32(M)``, bit for bit.  Returns ``(points float32 [*size, d], footprints float32 [*size, d, d], valid
    bool [*size])``."""
    size = [int(v) for v in np.atleast_1d(size)]
    d = len(size)
    Hm = np.asarray(H, dtype=np.float64)
    if Hm.shape != (d + 1, d + 1) or not np.isfinite(Hm).all():
        raise ValueError(f"projective_points: H must be a finite [{d + 1}, {d + 1}] array")
    if min(size) < 1:
        raise ValueError("projective_points: size needs entries >= 1")
    idx = np.stack(np.meshgrid(*[np.arange(e, dtype=np.float64) + 0.5 for e in size], indexing="ij"), axis=-1)
    with np.errstate(all="ignore"):
        s = idx @ Hm[d, :d] + Hm[d, d]
        valid = np.isfinite(s) & (s > 0)
        sv = np.where(valid, s, 1.0)
        A = Hm[:d]                                                                     # (warp_points' expression on [M | t])
        x = (idx @ A[:, :d].T + A[:, d]) / sv[..., None]
        J = (Hm[:d, :d] - x[..., :, None] * Hm[d, :d]) / sv[..., None, None]
    pts = np.where(valid[..., None], x, np.nan).astype(np.float32)
    foot = np.where(valid[..., None, None], J, 0.0).astype(np.float32)
    return pts, foot, valid


def map_footprints(points) -> np.ndarray:
    """The footprints of a dense lookup map (``Smoe.render_map``): ``points`` ``[*size, d]`` holds the source position of every
    output sample; column ``m`` of a sample's footprint is the central difference ``(p[i + e_m] - p[i - e_m]) * 0.5`` in
    float32, one-sided (``p[i + e_m] - p[i]`` / ``p[i] - p[i - e_m]``) at the ends of an axis and 0 on an axis of one sample.  A
    NaN neighbour makes the footprint non-finite, hence the sample void.  Returns float32 ``[*size, d, d]``."""
    p = np.asarray(points, dtype=np.float32)
    d = p.shape[-1] if p.ndim >= 1 else 0
    if p.ndim != d + 1 or d < 1:
        raise ValueError("map_footprints: points must be [*size, d] with d view axes")
    F = np.zeros(p.shape + (d,), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(d):
            E = p.shape[m]
            if E < 2:
                continue
            q = np.moveaxis(p, m, 0)
            col = np.empty_like(q)
            col[1:-1] = ((q[2:] - q[:-2]).astype(np.float32) * np.float32(0.5)).astype(np.float32)
            col[0] = q[1] - q[0]
            col[-1] = q[-1] - q[-2]
            F[..., m] = np.moveaxis(col, 0, m)
    return F


def to_planar(blocks: np.ndarray) -> np.ndarray:
    """(B, *block_shape, C) -> (B, C, N): the C-ABI target layout (include/smoe_hip.h)."""
    B, C = blocks.shape[0], blocks.shape[-1]
    N = int(np.prod(blocks.shape[1:-1]))           # explicit: a rank may hold no blocks at all (B = 0)
    return np.ascontiguousarray(blocks.reshape(B, N, C).transpose(0, 2, 1))


def from_planar(arr: np.ndarray, block_shape: Sequence[int]) -> np.ndarray:
    """(B, C, N) -> (B, *block_shape, C)."""
    B, C = arr.shape[0], arr.shape[1]
    return np.ascontiguousarray(arr.transpose(0, 2, 1)).reshape((B,) + tuple(block_shape) + (C,))


def get_batch_shape(desired_batches: int, joint_domain_shape: Sequence[int]) -> Tuple[int, ...]:
    """Smoe.get_batch_shape (smoe.py:2459-2543): the block shape used when no ``batch_size`` is given.
    Every axis is divided by one of its divisors so that the number of batches is the smallest
    possible count >= ``desired_batches``; among those the divisor tuple with the smallest sum
    (most cube-like split) wins, first hit in the reference's enumeration order on ties.
    ``joint_domain_shape`` = image shape incl. the trailing (d + C) axis, which is never split."""
    def divisors(n):
        factors = {}
        nn, i = n, 2
        while i * i <= nn:
            while nn % i == 0:
                factors[i] = factors.get(i, 0) + 1
                nn //= i
            i += 1
        if nn > 1:
            factors[nn] = 1
        primes = list(factors.keys())

        def generate(k):
            if k == len(primes):
                yield 1
            else:
                for factor in generate(k + 1):
                    p_i = 1
                    for _ in range(factors[primes[k]] + 1):
                        yield factor * p_i
                        p_i *= primes[k]
        return list(generate(0))

    import itertools
    shape = [int(v) for v in joint_domain_shape]
    factors = [divisors(n) for n in shape[:-1]] + [[1]]
    if len(shape) > 4:                                   # light-field hack of the reference (smoe.py:2507-2509)
        factors[0] = [1]
        factors[1] = [1]
    shapes = list(itertools.product(*factors))
    possible = np.array([float(np.prod(sh[:-1])) for sh in shapes])
    diff = possible - desired_batches
    diff[diff < 0] = np.inf
    aimed = possible[int(np.argmin(diff))]
    cand = [shapes[i] for i in np.where(possible == aimed)[0]]
    sums = [np.sum(divs[2:3]) if len(divs) > 4 else np.sum(divs) for divs in cand]
    divs = cand[int(np.argmin(sums))]
    return tuple(int(shape[i] / divs[i]) for i in range(len(shape)))


# ------------------------------------------------------------------------------------
# the reference's initialisers, per block
# ------------------------------------------------------------------------------------
def gen_domain_grid(kernels_per_dim: Sequence[int], dim: int) -> np.ndarray:
    """Smoe.gen_domain for a list input (smoe.py:2402-2415,2424): kernel centres with equal
    spacing between positions and the border."""
    kpd = [int(k) for k in kernels_per_dim]
    if len(kpd) == 1:
        kpd = kpd * dim
    coord = [np.linspace((1 / n) / 2, 1 - (1 / n) / 2, n) for n in kpd]
    grids = np.meshgrid(*coord, indexing="ij")
    return np.reshape(np.stack(grids, axis=-1), (int(np.prod(kpd)), dim))


def generate_kernel_grid(kernels_per_dim: Sequence[int], dim: int, train_inverse_cov: bool = False):
    """smoe.py:2146-2163 -> (musX_init (K,d), A_init (K,d,d))."""
    kpd = [int(k) for k in kernels_per_dim]
    mus = gen_domain_grid(kpd, dim)
    if len(kpd) > 1:
        A_proto = np.diag([2.0 * (k + 1) for k in kpd])
        K = int(np.prod(kpd))
    else:
        A_proto = np.zeros((dim, dim))
        np.fill_diagonal(A_proto, 2 * (kpd[0] + 1))
        K = kpd[0] ** dim
    A = np.tile(A_proto, (K, 1, 1))
    if train_inverse_cov:
        A = A ** 2
    return mus, A


def generate_experts(blocks: np.ndarray, musX_init: np.ndarray) -> np.ndarray:
    """smoe.py:2165-2235 per block -> nu_e_init (B,K,C): mean of the block's pixels inside
    the [mu - mu0, mu + mu0) window of every kernel (Python banker's ``round``)."""
    B = blocks.shape[0]
    shape = blocks.shape[1:-1]
    d = len(shape)
    K = musX_init.shape[0]
    stride = musX_init[0]
    nu = np.empty((B, K, blocks.shape[-1]), dtype=np.float32)
    for k in range(K):
        sl: List[slice] = [slice(None)]
        for ax in range(d):
            lo = int(round((musX_init[k, ax] - stride[ax]) * shape[ax]))
            hi = int(round((musX_init[k, ax] + stride[ax]) * shape[ax]))
            sl.append(slice(lo, hi))
        nu[:, k, :] = np.mean(blocks[tuple(sl)], axis=tuple(range(1, d + 1)))
    return nu


def init_block_params(blocks: np.ndarray, kernels_per_dim: Sequence[int], normalize_pis: bool = True,
                      train_inverse_cov: bool = False) -> Dict[str, np.ndarray]:
    """What Smoe.__init__ builds when no init_params are given (smoe.py:260-262), for every
    block: float32 arrays in the get_params() layout with a leading block axis."""
    B = blocks.shape[0]
    d = blocks.ndim - 2
    C = blocks.shape[-1]
    mus, A = generate_kernel_grid(kernels_per_dim, d, train_inverse_cov)
    K = mus.shape[0]
    pis = np.ones((K,), dtype=np.float32)          # generate_pis, smoe.py:2237-2242
    if normalize_pis:
        pis = pis / K
    return {
        "pis": np.ascontiguousarray(np.tile(pis, (B, 1))),
        "musX": np.ascontiguousarray(np.tile(mus.astype(np.float32), (B, 1, 1))),
        "A_diagonal": np.ascontiguousarray(np.tile(A.astype(np.float32), (B, 1, 1, 1))),
        "A_corr": np.zeros((B, K, d, d), dtype=np.float32),          # smoe.py:437
        "gamma_e": np.zeros((B, K, d, C), dtype=np.float32),         # smoe.py:2170
        "nu_e": generate_experts(blocks, mus),
    }


# ------------------------------------------------------------------------------------
# deterministic synthetic inputs
# ------------------------------------------------------------------------------------
def synthetic_blocks(B: int, block_shape: Sequence[int], C: int, seed: int) -> np.ndarray:
    """Random oriented step edge + linear ramp + N(0,(2/255)^2) noise per block, clipped,
    rounded to uint8 and divided by 255 (as utils.py:126-128 does).  (B, *block_shape, C) float32."""
    rng = np.random.default_rng(seed)
    d = len(block_shape)
    axes = [np.linspace(0, 1, s) for s in block_shape]
    grids = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
    normal = rng.normal(size=(B, d))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    offset = rng.uniform(0.25, 0.75, size=(B,))
    lo = rng.uniform(0.1, 0.9, size=(B, C))
    hi = rng.uniform(0.1, 0.9, size=(B, C))
    slope = rng.uniform(-0.3, 0.3, size=(B, d, C))
    out = np.empty((B,) + tuple(block_shape) + (C,), dtype=np.float32)
    step = 4096
    for s in range(0, B, step):
        e = min(B, s + step)
        nb = e - s
        proj = np.tensordot(grids - 0.5, normal[s:e].T, axes=([d], [0]))          # (*shape, nb)
        proj = np.moveaxis(proj, -1, 0) + 0.5
        side = (proj > offset[s:e].reshape((nb,) + (1,) * d)).astype(np.float64)
        ex = (nb,) + (1,) * d + (C,)
        img = lo[s:e].reshape(ex) * (1 - side[..., None]) + hi[s:e].reshape(ex) * side[..., None]
        img = img + np.einsum("...l,blc->b...c", grids - 0.5, slope[s:e])
        img = img + rng.normal(scale=2 / 255, size=img.shape)
        img = np.clip(img, 0, 1)
        out[s:e] = np.round(img * 255).astype(np.uint8).astype(np.float32) / np.float32(255.)
    return out


def psnr(mse, precision):
    """plotter.py:14-15: mse is mse_op, i.e. mean(diff^2) * (2^p)^2 (smoe.py:1053)."""
    return 10 * np.log10((2 ** precision) ** 2 / mse)
