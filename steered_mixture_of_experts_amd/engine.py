"""BlockEngine: thin host wrapper around the C ABI (include/smoe_hip.h).

PyTorch is used only as plumbing: device allocations, ``data_ptr()`` and the current HIP
stream.  All arithmetic happens in libsmoe_hip.so; there is no eager/PyTorch fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import blocks as blk

PARAM_NAMES = ("pis", "musX", "A_diagonal", "A_corr", "gamma_e", "nu_e")


@dataclasses.dataclass(kw_only=True)
class _CommonConfig:
    """The fields ``smoe_config`` and ``smoe_shared_config`` (include/smoe_hip.h) share; defaults = smoe_test.py CLI
    defaults with kernel adding off (smoe_test.py:262-352).  Keyword-only: the modes put their shapes in front."""
    channels: int
    kernels: int
    precision: int = 8
    margin: float = 0.5
    use_determinant: bool = True
    use_yuv: bool = False
    train_pis: bool = True
    train_gammas: bool = True
    train_musx: bool = True
    lr_expert: float = 1e-3
    lr_pis: float = 1e-5
    lr_steer: float = 1.0
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    grad_clip: float = 0.0
    pis_l1: float = 0.0
    u_l1: float = 0.0
    start_pis: int = 0
    only_y_gamma: bool = False
    ssim_opt: bool = False
    # fake-quantised variables in the graph (smoe.py:474-538); tuples ordered A, musX, nu_e, pis, gamma_e
    quantization_mode: int = 0
    quantize_pis: bool = False
    bit_depths: Sequence[int] = (20, 18, 6, 10, 10)
    lower_bounds: Sequence[float] = (-2500, -.3, -5, 0, -32)
    upper_bounds: Sequence[float] = (2500, 1.3, 5, 2, 32)
    train_inverse_cov: bool = False      # smoe.py:734-735,791-793 (reference ctor default True, CLI default False)
    radial_as: bool = False              # smoe.py:714-719: equal steering diagonals, tied gradient, A_corr untrained
    kernel_count_as_norm_l1: bool = False  # smoe.py:1022-1027: pis_l1 / count(qpis > 0)


@dataclasses.dataclass(kw_only=True)
class EngineConfig(_CommonConfig):
    """Mirror of ``smoe_config``: every block of ``block_shape`` pixels is its own model."""
    block_shape: Sequence[int]

    @property
    def dim(self) -> int:
        return len(self.block_shape)

    @property
    def pixels(self) -> int:
        n = 1
        for s in self.block_shape:
            n *= int(s)
        return n


@dataclasses.dataclass(kw_only=True)
class SharedConfig(_CommonConfig):
    """Mirror of ``smoe_shared_config``: ONE global kernel set over the image, batches of
    ``batch_shape`` pixels with per-batch kernel lists."""
    image_shape: Sequence[int]
    batch_shape: Sequence[int]
    overlap: int = 0

    @property
    def dim(self) -> int:
        return len(self.image_shape)


_AS_IS = ("channels", "kernels", "precision", "margin", "lr_expert", "lr_pis", "lr_steer", "beta1", "beta2", "adam_eps",
          "pis_l1", "u_l1")
_AS_INT = ("use_determinant", "use_yuv", "train_pis", "train_gammas", "train_musx", "only_y_gamma", "ssim_opt",
           "quantization_mode", "quantize_pis", "train_inverse_cov", "radial_as", "kernel_count_as_norm_l1")


def marshal_common(c, cfg: _CommonConfig):
    """Fill the fields a ``_lib.SmoeConfig`` / ``_lib.SmoeSharedConfig`` ``c`` takes from ``_CommonConfig`` (and ``dim``).
    The shapes, ``abi_version`` and ``device`` are the engine constructor's.  Pure ctypes: no device, no library."""
    c.dim = cfg.dim
    for name in _AS_IS:
        setattr(c, name, getattr(cfg, name))
    for name in _AS_INT:
        setattr(c, name, int(getattr(cfg, name)))
    c.grad_clip = cfg.grad_clip or 0.0
    c.start_pis = cfg.start_pis or cfg.kernels
    for i in range(5):
        c.bit_depths[i] = int(cfg.bit_depths[i])
        c.lower_bounds[i], c.upper_bounds[i] = float(cfg.lower_bounds[i]), float(cfg.upper_bounds[i])
    return c


def _shape3(dst, shape, d):
    """The first ``d`` entries of ``shape`` into a three-slot struct field, 1 for the axes the model does not have."""
    for i in range(3):
        dst[i] = int(shape[i]) if i < d else 1


def param_shapes(B: int, K: int, d: int, Cc: int) -> Dict[str, tuple]:
    """get_params() layout (smoe.py:1795-1800) with a leading block axis."""
    return {"pis": (B, K), "musX": (B, K, d), "A_diagonal": (B, K, d, d), "A_corr": (B, K, d, d),
            "gamma_e": (B, K, d, Cc), "nu_e": (B, K, Cc)}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class AdamState:
    """TF1 Adam slots on the device + the running beta powers on the host."""

    def __init__(self, params: Dict[str, torch.Tensor], beta1: float, beta2: float):
        self.m = {k: torch.zeros_like(v) for k, v in params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in params.items()}
        self.c = _lib.SmoeAdamState()
        self.c.beta1_power = beta1
        self.c.beta2_power = beta2
        self.c.step = 0

    @property
    def step(self) -> int:
        return int(self.c.step)


def _slots(ctype, values, fill):
    """A three-slot ctypes array: one entry per axis, ``fill`` for the axes the model does not have."""
    values = list(values)
    return (ctype * 3)(*(values + [fill] * (3 - len(values))))


class _Engine:
    """What the two engines share: library and device, the handle's life, the stream, the Adam slots and the argument
    plumbing of ``render``."""
    _name = _destroy = None        # the subclass's public name and the entry point that frees its handle

    def _open(self, cfg, device):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError(f"{self._name} needs a HIP device; this package has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.cfg = cfg

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(self.lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def new_adam_state(self, params: Dict[str, torch.Tensor]) -> AdamState:
        return AdamState(params, self.cfg.beta1, self.cfg.beta2)

    # -- render plumbing -----------------------------------------------------------
    def _check_render_arity(self, who, dtype, axes, others, needs):
        """The pixel type, and one entry per axis in ``axes`` and in each of ``others``.  ``who`` / ``needs``: the method's
        name and the wording of the arity in its message."""
        d = self.cfg.dim
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError("render: dtype must be torch.float32 or torch.uint8")
        if len(axes) != d or any(len(v) != d for v in others):
            raise ValueError(f"{who}: {needs} need {d} entries")

    def _check_axis_tables(self, who, axes, lengths=None):
        """Every axis table a float32 vector on the device, with ``lengths[l]`` entries (default: at least one)."""
        for l, t in enumerate(axes):
            if t.dim() != 1 or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device \
                    or (t.numel() < 1 if lengths is None else t.numel() != lengths[l]):
                raise ValueError(f"{who}: every axis table must be a contiguous 1-d float32 tensor on {self.device}"
                                 + ("" if lengths is None else f" with grid * samples entries ({lengths})"))

    def _render_planes(self, out, extent, dtype, everything: bool, want_argmax: bool, none, id_dtype):
        """The image ``[*extent, C]`` to render into -- ``out`` checked, or a new one (zero-filled unless the call renders
        ``everything``) --, the pixel format constant of ``dtype``, and the kernel-id map ``[*extent]`` filled with
        ``none`` (or None)."""
        shape = tuple(extent) + (self.cfg.channels,)
        if out is None:
            out = (torch.empty if everything else torch.zeros)(shape, dtype=dtype, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"render: out must be a contiguous {dtype} tensor {shape} on {self.device}")
        am = torch.full(tuple(extent), none, dtype=id_dtype, device=self.device) if want_argmax else None
        return out, (_lib.SMOE_IMAGE_U8 if dtype == torch.uint8 else _lib.SMOE_IMAGE_F32), am

    def _blend_list(self, who, blend):
        """``blend`` as one float per axis (a single value stands for every axis), or None."""
        if blend is None:
            return None
        d = self.cfg.dim
        bl = [float(v) for v in np.atleast_1d(blend)]
        bl = bl * d if len(bl) == 1 else bl
        if len(bl) != d:
            raise ValueError(f"{who}: blend needs one value or {d}")
        return bl

    @staticmethod
    def _axis_slots(axes):
        return _slots(C.c_void_p, [t.data_ptr() for t in axes], None)


class BlockEngine(_Engine):
    _name, _destroy = "BlockEngine", "smoe_destroy"

    def __init__(self, cfg: EngineConfig, device: Optional[torch.device] = None):
        self._open(cfg, device)
        c = marshal_common(_lib.SmoeConfig(), cfg)
        c.abi_version = _lib.SMOE_ABI_VERSION
        c.device = self.device.index or 0
        _shape3(c.block_shape, cfg.block_shape, cfg.dim)
        self._c = c
        self._h = C.c_void_p()
        _lib.check(self.lib.smoe_create(C.byref(self._h), C.byref(c)))

    # -- helpers ---------------------------------------------------------------
    def _check_params(self, p: Dict[str, torch.Tensor], B: int):
        shapes = param_shapes(B, self.cfg.kernels, self.cfg.dim, self.cfg.channels)
        for name in PARAM_NAMES:
            t = p[name]
            if tuple(t.shape) != shapes[name] or t.dtype != torch.float32 or not t.is_contiguous() \
                    or t.device != self.device:
                raise ValueError(f"parameter {name}: expected contiguous float32 {shapes[name]} on {self.device}, "
                                 f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    def _cparams(self, p: Dict[str, torch.Tensor]) -> _lib.SmoeParams:
        s = _lib.SmoeParams()
        for name in PARAM_NAMES:
            setattr(s, name, p[name].data_ptr())
        return s

    def _check_target(self, target: torch.Tensor, loss_w: Optional[torch.Tensor]) -> int:
        if target.dim() != 3 or target.shape[1] != self.cfg.channels or target.shape[2] != self.cfg.pixels \
                or target.dtype != torch.float32 or not target.is_contiguous() or target.device != self.device:
            raise ValueError(f"target must be contiguous float32 [B,{self.cfg.channels},{self.cfg.pixels}] on {self.device}")
        B = target.shape[0]
        if loss_w is not None and (tuple(loss_w.shape) != (B, self.cfg.pixels) or loss_w.dtype != torch.float32
                                   or not loss_w.is_contiguous() or loss_w.device != self.device):
            raise ValueError("loss_w must be contiguous float32 [B,N]")
        return B

    def new_params(self, B: int) -> Dict[str, torch.Tensor]:
        shapes = param_shapes(B, self.cfg.kernels, self.cfg.dim, self.cfg.channels)
        return {k: torch.zeros(s, dtype=torch.float32, device=self.device) for k, s in shapes.items()}

    def coords(self) -> torch.Tensor:
        out = torch.empty((self.cfg.dim, self.cfg.pixels), dtype=torch.float32)
        _lib.check(self.lib.smoe_get_coords(self._h, C.c_void_p(out.data_ptr())))
        return out

    def set_tiling(self, lanes_per_block: int):
        _lib.check(self.lib.smoe_set_tiling(self._h, lanes_per_block))

    def set_total_blocks(self, total_blocks: int):
        """Block count of the WHOLE job the calls of this engine are shards of (0 = each call's own count): the kernel
        tiling -- and with it the summation order inside a block -- is then the same for every split of the job over
        calls / ranks, so per-block results are bit-identical (include/smoe_hip.h: smoe_set_total_blocks)."""
        _lib.check(self.lib.smoe_set_total_blocks(self._h, int(total_blocks)))

    def set_center_grid(self, grid: Optional[torch.Tensor]):
        """use_diff_center with quantization_mode 2 / 3: the kernel-grid centres [B, K, d] (float32, on the device, laid
        out like musX) the trained offsets are relative to, or None to clear.  The engine keeps a reference."""
        if grid is not None:
            assert grid.dtype == torch.float32 and grid.is_contiguous() and grid.device == self.device
            assert grid.ndim == 3 and tuple(grid.shape[1:]) == (self.cfg.kernels, len(self.cfg.block_shape))
        self._center_grid = grid
        _lib.check(self.lib.smoe_set_center_grid(self._h, _ptr(grid)))

    def fit_occupancy(self, B: int) -> int:
        return int(self.lib.smoe_fit_occupancy(self._h, B))

    def fit_variant(self, B: int) -> str:
        return self.lib.smoe_fit_variant(self._h, B).decode()

    def last_fit_variant(self) -> str:
        """Name of the kernel the last ``fit`` launched, with its tiling / graph / loss-weight marks (include/smoe_hip.h:
        smoe_last_fit_variant); "" before the first launch."""
        return self.lib.smoe_last_fit_variant(self._h).decode()

    # -- the hot path ------------------------------------------------------------
    def forward(self, target, params, active, loss_w=None, want_recon=True, want_argmax=False,
                want_gate=False, update_active=True):
        B = self._check_target(target, loss_w)
        self._check_params(params, B)
        dev = self.device
        N, K, Cc = self.cfg.pixels, self.cfg.kernels, self.cfg.channels
        out = {
            "loss": torch.empty((B,), dtype=torch.float32, device=dev),
            "sse": torch.empty((B,), dtype=torch.float32, device=dev),
            "recon": torch.empty((B, Cc, N), dtype=torch.float32, device=dev) if want_recon else None,
            "argmax": torch.empty((B, N), dtype=torch.uint8, device=dev) if want_argmax else None,
            "gate_w": torch.empty((B, K, N), dtype=torch.float32, device=dev) if want_gate else None,
        }
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_forward(self._h, B, _ptr(target), _ptr(loss_w), C.byref(cp),
                                         _ptr(out["recon"]), _ptr(out["argmax"]), _ptr(out["gate_w"]),
                                         _ptr(out["loss"]), _ptr(out["sse"]), _ptr(active),
                                         int(update_active), self._stream()))
        return out

    def _render(self, who, entry, params, active, covered, axes, grid, extent, first_block, B, out, dtype, want_argmax,
                blend=None):
        """``render`` and ``render_blend``: ``who`` names the method in the messages, ``entry`` is its C entry point.
        ``covered``: the blocks ``params`` and ``active`` hold; ``B``: the blocks to render; ``blend``: render_blend's."""
        self._check_params(params, covered)
        self._check_render_arity(who, dtype, axes, (grid, extent), "axes, grid and extent")
        self._check_axis_tables(who, axes)
        bl = self._blend_list(who, blend)
        grid = [int(g) for g in grid]
        extent = [int(e) for e in extent]
        total = 1
        for g in grid:
            total *= g
        if active is not None and (tuple(active.shape) != (covered,) or active.dtype != torch.int32 or active.device != self.device):
            raise ValueError(f"{who}: active must be int32 [{covered}] on {self.device}")
        out, fmt, am = self._render_planes(out, extent, dtype, first_block == 0 and B == total, want_argmax, 255, torch.uint8)
        if B > 0:
            cp = self._cparams(params)
            args = [self._h, int(first_block), B, C.byref(cp), _ptr(active), self._axis_slots(axes),
                    _slots(C.c_int32, [int(t.numel()) for t in axes], 1), _slots(C.c_int32, grid, 1), _slots(C.c_int64, extent, 1)]
            if blend is not None:
                args.append(_slots(C.c_float, bl, 0.0))
            _lib.check(entry(*args, _ptr(out), fmt, _ptr(am), self._stream()))
        return (out, am) if want_argmax else out

    def render(self, params, active, axes, grid, extent, first_block=0, out=None, dtype=torch.float32,
               want_argmax=False):
        """Decode: evaluate the blocks ``[first_block, first_block + B)`` of an image-wide block ``grid`` on the separable
        sample grid ``axes`` (one float32 device table per axis, block units) into the stitched image
        ``[*extent, C]`` (include/smoe_hip.h: smoe_render).  ``active`` [B] int32 or None (every kernel listed).  ``out``: a
        full-size image to render into (only the positions of the rendered blocks are written); otherwise a new one,
        zero-filled where this call renders only a part.  Returns the image, with ``want_argmax`` also the uint8 kernel
        map ``[*extent]`` (255: no kernel has influence; 255 as well where no block was rendered)."""
        B = int(params["pis"].shape[0])
        return self._render("render", self.lib.smoe_render, params, active, B, axes, grid, extent, first_block, B, out, dtype,
                            want_argmax)

    def render_blend(self, params, active, axes, grid, extent, blend, first_block=0, num_blocks=None, out=None,
                     dtype=torch.float32, want_argmax=False, center_grid=None):
        """Seam-free decode (include/smoe_hip.h: smoe_render_blend): ``render``, with the neighbouring blocks' models
        cross-faded in a band of ``blend[l]`` source pixels (half-width, ``0 .. block_shape[l] / 2``) around every block
        border.  Unlike ``render``, ``params`` and ``active`` cover ALL ``prod(grid)`` blocks of the image -- the neighbours
        of the rendered range ``[first_block, first_block + num_blocks)`` (default: up to the last block) are read --
        and so does ``center_grid`` [prod(grid), K, d], the image-wide kernel grid of a use_diff_center model whose
        engine holds a shard's grid (it is put back afterwards).  Returns what ``render`` returns."""
        total = 1
        for g in grid:
            total *= int(g)
        B = total - int(first_block) if num_blocks is None else int(num_blocks)

        def entry(*args):
            with self._center_grid_installed(center_grid):
                return self.lib.smoe_render_blend(*args)
        return self._render("render_blend", entry, params, active, total, axes, grid, extent, first_block, B, out, dtype,
                            want_argmax, blend)

    def render_view(self, params, active, grid, view_first, starts, axes, blend=None, out=None, dtype=torch.float32,
                    want_argmax=False, center_grid=None):
        """Viewport decode (include/smoe_hip.h: smoe_render_view): the window of the image that the per-axis tables describe,
        into a dense image ``[E_0, E_1(, E_2), C]``.  ``starts[l]``: HOST int32 table of ``view_blocks[l] + 1`` entries
        (samples ``[start[j], start[j + 1])`` lie in block ``view_first[l] + j``; ``start[-1] = E_l``); ``axes[l]``: float32
        device table of the ``E_l`` coordinates in block units (``blocks.view_axis`` makes both).  ``params``, ``active`` and
        ``center_grid`` cover ALL ``prod(grid)`` blocks, as in ``render_blend``; ``blend``: None or render_blend's.  Returns
        the image, with ``want_argmax`` also the uint8 map of the own block's kernel ids (255: none)."""
        who = "render_view"
        grid = [int(g) for g in grid]
        view_first = [int(g) for g in view_first]
        self._check_render_arity(who, dtype, axes, (grid, view_first, starts), "axes, grid, view_first and starts")
        total = 1
        for g in grid:
            total *= g
        self._check_params(params, total)
        if active is not None and (tuple(active.shape) != (total,) or active.dtype != torch.int32 or active.device != self.device):
            raise ValueError(f"{who}: active must be int32 [{total}] on {self.device}")
        st = [np.ascontiguousarray(np.asarray(t), dtype=np.int32) for t in starts]
        if any(t.ndim != 1 or t.size < 2 for t in st):
            raise ValueError(f"{who}: every start table needs view_blocks + 1 >= 2 entries")
        extent = [int(t[-1]) for t in st]
        if min(extent) < 1:
            raise ValueError(f"{who}: every axis needs at least one sample")
        self._check_axis_tables(who, axes, extent)
        bl = self._blend_list(who, blend)
        out, fmt, am = self._render_planes(out, extent, dtype, True, want_argmax, 255, torch.uint8)
        cp = self._cparams(params)
        with self._center_grid_installed(center_grid):
            rc = self.lib.smoe_render_view(
                self._h, C.byref(cp), _ptr(active), _slots(C.c_int32, grid, 1), _slots(C.c_int32, view_first, 0),
                _slots(C.c_int32, [t.size - 1 for t in st], 1), _slots(C.c_void_p, [t.ctypes.data for t in st], None),
                self._axis_slots(axes), None if bl is None else _slots(C.c_float, bl, 0.0), _ptr(out), fmt, _ptr(am),
                self._stream())
        _lib.check(rc)
        return (out, am) if want_argmax else out

    @contextlib.contextmanager
    def _center_grid_installed(self, center_grid):
        """The image-wide centre grid (or None: nothing to do) around a launch alone: what the engine held is put back."""
        if center_grid is None:
            yield
            return
        held = getattr(self, "_center_grid", None)
        self.set_center_grid(center_grid)
        try:
            yield
        finally:
            self.set_center_grid(held)

    def _check_point_args(self, who, params, active, grid, length, points, blend):
        """The arguments ``sample`` and ``sample_grad`` share, checked (``grid`` and ``length``: lists of int).  Returns the
        number of points and the blend as one float per axis (or None)."""
        d = self.cfg.dim
        if len(grid) != d or len(length) != d:
            raise ValueError(f"{who}: grid and length need {d} entries")
        total = 1
        for g in grid:
            total *= g
        self._check_params(params, total)
        if active is not None and (tuple(active.shape) != (total,) or active.dtype != torch.int32 or active.device != self.device):
            raise ValueError(f"{who}: active must be int32 [{total}] on {self.device}")
        if points.dim() != 2 or points.shape[1] != d or points.dtype != torch.float32 or not points.is_contiguous() \
                or points.device != self.device:
            raise ValueError(f"{who}: points must be a contiguous float32 tensor [N, {d}] on {self.device}")
        bl = self._blend_list(who, blend)
        return int(points.shape[0]), bl

    def _point_out(self, who, out, shape, dtype, dtype_name):
        """``out`` checked against ``shape`` and ``dtype`` (``dtype_name``: its wording in the message), or a new tensor."""
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"{who}: out must be a contiguous {dtype_name} tensor {shape} on {self.device}")
        return out

    def sample(self, params, active, grid, length, points, blend=None, out=None, dtype=torch.float32, want_argmax=False,
               want_block=False, center_grid=None):
        """Point decode (include/smoe_hip.h: smoe_sample): the model at the positions ``points`` -- a contiguous float32 device
        tensor ``[N, d]`` in source pixels (``blocks.point_blocks`` states the mapping) -- into ``[N, C]``.  ``length``: the
        true extent of the image in pixels per axis.  ``params``, ``active`` and ``center_grid`` cover ALL ``prod(grid)``
        blocks, as in ``render_view``; ``blend``: None or render_blend's.  Points outside the image give 0.  Returns the
        values, then with ``want_argmax`` the uint8 local kernel ids of the own block ``[N]`` (255: none or outside) and with
        ``want_block`` the int32 image-wide block indices ``[N]`` (-1: outside)."""
        who = "sample"
        grid, length = [int(g) for g in grid], [int(v) for v in length]
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{who}: dtype must be torch.float32 or torch.uint8")
        N, bl = self._check_point_args(who, params, active, grid, length, points, blend)
        out = self._point_out(who, out, (N, self.cfg.channels), dtype, dtype)
        fmt = _lib.SMOE_IMAGE_U8 if dtype == torch.uint8 else _lib.SMOE_IMAGE_F32
        am = torch.empty((N,), dtype=torch.uint8, device=self.device) if want_argmax else None
        bk = torch.empty((N,), dtype=torch.int32, device=self.device) if want_block else None
        cp = self._cparams(params)
        with self._center_grid_installed(center_grid):
            rc = self.lib.smoe_sample(self._h, C.byref(cp), _ptr(active), _slots(C.c_int32, grid, 1), _slots(C.c_int32, length, 1),
                                      _ptr(points), N, None if bl is None else _slots(C.c_float, bl, 0.0), _ptr(out), fmt,
                                      _ptr(am), _ptr(bk), self._stream())
        _lib.check(rc)
        res = (out,) + ((am,) if want_argmax else ()) + ((bk,) if want_block else ())
        return res if len(res) > 1 else out

    def sample_grad(self, params, active, grid, length, points, blend=None, out=None, want_values=False, want_block=False,
                    center_grid=None):
        """Point derivative (include/smoe_hip.h: smoe_sample_grad): the exact spatial derivative of the model at the positions
        ``points`` -- ``sample``'s points, blocks, lists, ``center_grid`` and ``blend`` -- into ``[N, d, C]`` float32:
        ``jac[i, l, c] = dV_c / dx_l`` per source pixel, of the value before the lattice.  Points outside the image give 0.
        Returns the Jacobian, then with ``want_values`` the float32 values before the lattice ``[N, C]`` and with
        ``want_block`` the int32 image-wide block indices ``[N]`` (-1: outside)."""
        who = "sample_grad"
        grid, length = [int(g) for g in grid], [int(v) for v in length]
        N, bl = self._check_point_args(who, params, active, grid, length, points, blend)
        out = self._point_out(who, out, (N, self.cfg.dim, self.cfg.channels), torch.float32, "float32")
        val = torch.empty((N, self.cfg.channels), dtype=torch.float32, device=self.device) if want_values else None
        bk = torch.empty((N,), dtype=torch.int32, device=self.device) if want_block else None
        cp = self._cparams(params)
        with self._center_grid_installed(center_grid):
            rc = self.lib.smoe_sample_grad(self._h, C.byref(cp), _ptr(active), _slots(C.c_int32, grid, 1),
                                           _slots(C.c_int32, length, 1), _ptr(points), N,
                                           None if bl is None else _slots(C.c_float, bl, 0.0), _ptr(out), _ptr(val), _ptr(bk),
                                           self._stream())
        _lib.check(rc)
        res = (out,) + ((val,) if want_values else ()) + ((bk,) if want_block else ())
        return res if len(res) > 1 else out

    def sample_area(self, params, active, grid, length, points, footprint, taps, blend=None, out=None, dtype=torch.float32,
                    want_mean=False, want_count=False, want_block=False, center_grid=None):
        """Anti-aliased point decode (include/smoe_hip.h: smoe_sample_area): per point -- the centre of an output cell, as
        ``sample``'s points -- the mean of the model over a regular grid of ``taps[m]`` taps along view axis ``m`` inside the
        cell's ``footprint`` (host ``[d, d]``, column ``m`` = the cell's edge vector along view axis ``m`` in source pixels;
        ``blocks.area_taps`` states the positions), put on the lattice, into ``[N, C]``.  Taps outside the image are left out
        of the mean.  ``params``, ``active``, ``center_grid`` and ``blend`` are ``sample``'s.  Returns the lattice values, then
        with ``want_mean`` the float32 means before the lattice ``[N, C]``, with ``want_count`` the uint8 number of taps
        inside ``[N]`` and with ``want_block`` the int32 own block of the centre ``[N]`` (-1: outside)."""
        who = "sample_area"
        grid, length = [int(g) for g in grid], [int(v) for v in length]
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{who}: dtype must be torch.float32 or torch.uint8")
        N, bl = self._check_point_args(who, params, active, grid, length, points, blend)
        d = self.cfg.dim
        try:
            F, tp = blk.area_args(footprint, taps, d)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        out = self._point_out(who, out, (N, self.cfg.channels), dtype, dtype)
        fmt = _lib.SMOE_IMAGE_U8 if dtype == torch.uint8 else _lib.SMOE_IMAGE_F32
        mean = torch.empty((N, self.cfg.channels), dtype=torch.float32, device=self.device) if want_mean else None
        cnt = torch.empty((N,), dtype=torch.uint8, device=self.device) if want_count else None
        bk = torch.empty((N,), dtype=torch.int32, device=self.device) if want_block else None
        cp = self._cparams(params)
        with self._center_grid_installed(center_grid):
            rc = self.lib.smoe_sample_area(self._h, C.byref(cp), _ptr(active), _slots(C.c_int32, grid, 1),
                                           _slots(C.c_int32, length, 1), _ptr(points), N,
                                           (C.c_float * (d * d))(*[float(v) for v in F.reshape(-1)]), (C.c_int32 * d)(*tp),
                                           None if bl is None else _slots(C.c_float, bl, 0.0), _ptr(out), fmt, _ptr(mean),
                                           _ptr(cnt), _ptr(bk), self._stream())
        _lib.check(rc)
        res = (out,) + ((mean,) if want_mean else ()) + ((cnt,) if want_count else ()) + ((bk,) if want_block else ())
        return res if len(res) > 1 else out

    def sample_area_each(self, params, active, grid, length, points, footprints, taps, blend=None, out=None, dtype=torch.float32,
                         want_mean=False, want_count=False, want_block=False, center_grid=None):
        """Anti-aliased point decode with a footprint of its own per point (include/smoe_hip.h: smoe_sample_area_each):
        ``sample_area`` where point ``i`` has the footprint ``footprints[i]`` and the tap counts ``taps[i]`` -- contiguous
        device tensors, float32 ``[N, d, d]`` and uint8 ``[N, d]`` (``blocks.area_taps_each`` states the positions).  A point
        whose taps are outside 1 .. 16, multiply to more than 64 or whose footprint is not finite is void: 0 / 0 / count 0.
        Everything else, and what is returned, is ``sample_area``'s."""
        who = "sample_area_each"
        grid, length = [int(g) for g in grid], [int(v) for v in length]
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{who}: dtype must be torch.float32 or torch.uint8")
        N, bl = self._check_point_args(who, params, active, grid, length, points, blend)
        d = self.cfg.dim
        if not torch.is_tensor(footprints) or tuple(footprints.shape) != (N, d, d) or footprints.dtype != torch.float32 \
                or not footprints.is_contiguous() or footprints.device != self.device:
            raise ValueError(f"{who}: footprints must be a contiguous float32 tensor [{N}, {d}, {d}] on {self.device}")
        if not torch.is_tensor(taps) or tuple(taps.shape) != (N, d) or taps.dtype != torch.uint8 or not taps.is_contiguous() \
                or taps.device != self.device:
            raise ValueError(f"{who}: taps must be a contiguous uint8 tensor [{N}, {d}] on {self.device}")
        out = self._point_out(who, out, (N, self.cfg.channels), dtype, dtype)
        fmt = _lib.SMOE_IMAGE_U8 if dtype == torch.uint8 else _lib.SMOE_IMAGE_F32
        mean = torch.empty((N, self.cfg.channels), dtype=torch.float32, device=self.device) if want_mean else None
        cnt = torch.empty((N,), dtype=torch.uint8, device=self.device) if want_count else None
        bk = torch.empty((N,), dtype=torch.int32, device=self.device) if want_block else None
        cp = self._cparams(params)
        with self._center_grid_installed(center_grid):
            rc = self.lib.smoe_sample_area_each(self._h, C.byref(cp), _ptr(active), _slots(C.c_int32, grid, 1),
                                                _slots(C.c_int32, length, 1), _ptr(points), N, _ptr(footprints), _ptr(taps),
                                                None if bl is None else _slots(C.c_float, bl, 0.0), _ptr(out), fmt, _ptr(mean),
                                                _ptr(cnt), _ptr(bk), self._stream())
        _lib.check(rc)
        res = (out,) + ((mean,) if want_mean else ()) + ((cnt,) if want_count else ()) + ((bk,) if want_block else ())
        return res if len(res) > 1 else out

    def fit(self, target, params, state: AdamState, active, n_iters: int, loss_w=None, diverged=None,
            loss0=None, loss_out=None, sse_out=None, loss_w_is_sample=False):
        """loss_w_is_sample: ``loss_w`` is a pixel sub-sample (N / n for the drawn pixels, 0 otherwise; smoe.py:1664-1667):
        the pixels with weight 0 are "not fed" and do not vote in the kernel-list prune (include/smoe_hip.h: smoe_set_sampling)."""
        B = self._check_target(target, loss_w)
        _lib.check(self.lib.smoe_set_sampling(self._h, int(bool(loss_w_is_sample))))
        self._check_params(params, B)
        self._check_params(state.m, B)
        self._check_params(state.v, B)
        state.c.m = self._cparams(state.m)
        state.c.v = self._cparams(state.v)
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_fit(self._h, B, _ptr(target), _ptr(loss_w), C.byref(cp), C.byref(state.c),
                                     int(n_iters), _ptr(loss_out), _ptr(sse_out), _ptr(active), _ptr(diverged),
                                     _ptr(loss0), self._stream()))

    def prepare_fit(self, target, params, state: AdamState, active, loss_w=None, diverged=None, loss0=None, loss_out=None,
                    sse_out=None, loss_w_is_sample=False):
        """``fit`` with the argument checks and the ctypes marshalling done once: returns ``run(n_iters)`` that only makes the
        C call (a few microseconds of host time per launch instead of the ~50 of the checked path).  The tensors must stay
        alive and in place while ``run`` is used (measurement loops, bench.py)."""
        B = self._check_target(target, loss_w)
        self._check_params(params, B)
        self._check_params(state.m, B)
        self._check_params(state.v, B)
        state.c.m = self._cparams(state.m)
        state.c.v = self._cparams(state.v)
        cp = self._cparams(params)
        args = (_ptr(target), _ptr(loss_w), C.byref(cp), C.byref(state.c))
        tail = (_ptr(loss_out), _ptr(sse_out), _ptr(active), _ptr(diverged), _ptr(loss0), self._stream())
        fit, h, sample = self.lib.smoe_fit, self._h, int(bool(loss_w_is_sample))
        keep = (cp, target, loss_w, params, state, active, diverged, loss0, loss_out, sse_out)

        def run(n_iters: int, _keep=keep):
            _lib.check(self.lib.smoe_set_sampling(h, sample))
            _lib.check(fit(h, B, *args, int(n_iters), *tail))
        return run

    def update_kernel_list(self, params, active):
        B = active.shape[0]
        self._check_params(params, B)
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_update_kernel_list(self._h, B, C.byref(cp), _ptr(active), self._stream()))

    def checkpoint_best(self, loss, best_loss, params, best):
        B = loss.shape[0]
        self._check_params(params, B)
        self._check_params(best, B)
        cp, cb = self._cparams(params), self._cparams(best)
        _lib.check(self.lib.smoe_checkpoint_best(self._h, B, _ptr(loss), _ptr(best_loss), C.byref(cp),
                                                 C.byref(cb), self._stream()))

    def reduce_scalars(self, loss, sse, active) -> torch.Tensor:
        """[sum loss*N, sum sse, sum popcount(active)] as a float64 device tensor."""
        out = torch.empty((3,), dtype=torch.float64, device=self.device)
        B = 0
        for t in (loss, sse, active):
            if t is not None:
                B = t.shape[0]
        _lib.check(self.lib.smoe_reduce_scalars(self._h, B, _ptr(loss), _ptr(sse), _ptr(active), _ptr(out),
                                                self._stream()))
        return out


# =====================================================================================================
# shared-kernel image mode
# =====================================================================================================
class SharedEngine(_Engine):
    """Host wrapper of the smoe_shared_* entry points.  Parameters: dict of contiguous float32
    device tensors in the get_params() layout with leading K (no block axis)."""
    _name, _destroy = "SharedEngine", "smoe_shared_destroy"

    def __init__(self, cfg: SharedConfig, device: Optional[torch.device] = None):
        self._open(cfg, device)
        c = marshal_common(_lib.SmoeSharedConfig(), cfg)
        c.abi_version, c.device = _lib.SMOE_ABI_VERSION, self.device.index or 0
        _shape3(c.image_shape, cfg.image_shape, cfg.dim)
        _shape3(c.batch_shape, cfg.batch_shape, cfg.dim)
        c.overlap = int(cfg.overlap)
        self._h = C.c_void_p()
        _lib.check(self.lib.smoe_shared_create(C.byref(self._h), C.byref(c)))
        self.num_batches = int(self.lib.smoe_shared_num_batches(self._h))
        self.list_words = int(self.lib.smoe_shared_list_words(self._h))
        self.batch_pixels = 1
        for b in cfg.batch_shape:
            self.batch_pixels *= int(b)

    def _cparams(self, p):
        shapes = param_shapes(1, self.cfg.kernels, self.cfg.dim, self.cfg.channels)
        s = _lib.SmoeParams()
        for name in PARAM_NAMES:
            t = p[name]
            if tuple(t.shape) != shapes[name][1:] or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"parameter {name}: expected contiguous float32 {shapes[name][1:]} on {self.device}")
            setattr(s, name, t.data_ptr())
        return s

    def new_lists(self, nb: Optional[int] = None) -> torch.Tensor:
        """All kernels listed in every batch (smoe.py:315)."""
        nb = self.num_batches if nb is None else nb
        K, KW = self.cfg.kernels, self.list_words
        words = torch.full((nb, KW), -1, dtype=torch.int32, device=self.device)
        if K % 32:
            words[:, KW - 1] = (1 << (K % 32)) - 1
        return words

    def _check_target(self, target, nb):
        want = (nb, self.cfg.channels, self.batch_pixels)
        if tuple(target.shape) != want or target.dtype != torch.float32 or not target.is_contiguous():
            raise ValueError(f"target must be contiguous float32 {want}")

    def forward(self, target, params, lists, first_batch=0, want_recon=True, want_argmax=False, update_lists=True):
        nb = lists.shape[0]
        self._check_target(target, nb)
        dev = self.device
        out = {"loss": torch.empty((nb,), dtype=torch.float32, device=dev),
               "sse": torch.empty((nb,), dtype=torch.float32, device=dev),
               "recon": torch.empty_like(target) if want_recon else None,
               "argmax": torch.empty((nb, self.batch_pixels), dtype=torch.int32, device=dev) if want_argmax else None}
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_shared_forward(self._h, first_batch, nb, _ptr(target), C.byref(cp), _ptr(out["recon"]),
                                                _ptr(out["argmax"]), _ptr(out["loss"]), _ptr(out["sse"]), _ptr(lists),
                                                int(update_lists), self._stream()))
        return out

    def render(self, params, lists, axes, samples, first_batch=0, out=None, dtype=torch.float32, want_argmax=False,
               num_batches=None):
        """Decode: evaluate the batches ``[first_batch, first_batch + nb)`` on the separable sample grid ``axes`` (one
        float32 device table per IMAGE axis with ``grid_l * samples[l]`` coordinates in image units) into the interleaved
        image ``[*E, C]``, ``E_l = grid_l * samples[l]`` (include/smoe_hip.h: smoe_shared_render).  ``lists`` [nb, KW] int32
        (row 0 = batch ``first_batch``, only read) or None: every kernel, ``nb`` then comes from ``num_batches`` (default:
        all batches from ``first_batch`` on).  ``out``: a full-size image to render into (only the positions of the
        rendered batches are written); otherwise a new one, zero-filled where this call renders only a part.  Returns the
        image, with ``want_argmax`` also the int32 map ``[*E]`` of global kernel ids (-1: no kernel has influence on the
        sample; -1 as well where no batch was rendered)."""
        self._check_render_arity("render", dtype, axes, (samples,), "axes and samples")
        samples = [int(m) for m in samples]
        if min(samples) < 1:
            raise ValueError("render: at least one sample per batch and axis")
        grid = [int(s) // int(b) for s, b in zip(self.cfg.image_shape, self.cfg.batch_shape)]
        extent = [g * m for g, m in zip(grid, samples)]
        self._check_axis_tables("render", axes, extent)
        if lists is not None:
            nb = int(lists.shape[0])
            if (tuple(lists.shape) != (nb, self.list_words) or lists.dtype != torch.int32 or not lists.is_contiguous()
                    or lists.device != self.device):
                raise ValueError(f"render: lists must be a contiguous int32 [nb, {self.list_words}] tensor on {self.device}")
        else:
            nb = self.num_batches - int(first_batch) if num_batches is None else int(num_batches)
        if first_batch < 0 or nb < 0 or first_batch + nb > self.num_batches:
            raise ValueError("render: batch range out of bounds")
        out, fmt, am = self._render_planes(out, extent, dtype, nb == self.num_batches, want_argmax, -1, torch.int32)
        if nb > 0:
            cp = self._cparams(params)
            _lib.check(self.lib.smoe_shared_render(self._h, int(first_batch), nb, C.byref(cp), _ptr(lists), self._axis_slots(axes),
                                                   _slots(C.c_int32, samples, 1), _ptr(out), fmt, _ptr(am), self._stream()))
        return (out, am) if want_argmax else out

    def _check_all_lists(self, who, lists):
        """``lists`` of ALL batches, as the point and viewport decoders index them (global batch id), or None."""
        want = (self.num_batches, self.list_words)
        if lists is not None and (tuple(lists.shape) != want or lists.dtype != torch.int32 or not lists.is_contiguous()
                                  or lists.device != self.device):
            raise ValueError(f"{who}: lists must be a contiguous int32 {list(want)} tensor on {self.device} (all batches)")

    def _dense_planes(self, who, shape, out, dtype, want_argmax):
        """The value plane ``[*shape, C]`` (``out`` checked, or a new one), its format constant and the id plane or None."""
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{who}: dtype must be torch.float32 or torch.uint8")
        full = tuple(shape) + (self.cfg.channels,)
        if out is None:
            out = torch.empty(full, dtype=dtype, device=self.device)
        elif tuple(out.shape) != full or out.dtype != dtype or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"{who}: out must be a contiguous {dtype} tensor {full} on {self.device}")
        am = torch.empty(tuple(shape), dtype=torch.int32, device=self.device) if want_argmax else None
        return out, (_lib.SMOE_IMAGE_U8 if dtype == torch.uint8 else _lib.SMOE_IMAGE_F32), am

    def sample(self, params, lists, points, out=None, dtype=torch.float32, want_argmax=False):
        """Point decode (include/smoe_hip.h: smoe_shared_sample): the model at the positions ``points`` -- a contiguous float32
        device tensor ``[N, d]`` in source pixels (``blocks.point_blocks`` states the mapping) -- into ``[N, C]``, every point
        with the kernel list of the batch that owns it.  ``lists`` int32 ``[num_batches, KW]`` of ALL batches (only read) or
        None: every kernel.  Points outside the image give 0.  Returns the values, with ``want_argmax`` also the int32 global
        kernel ids ``[N]`` (-1: no kernel has influence, or outside)."""
        who = "sample"
        N = self._check_points(who, points, lists)
        out, fmt, am = self._dense_planes(who, (N,), out, dtype, want_argmax)
        if N > 0:
            cp = self._cparams(params)
            _lib.check(self.lib.smoe_shared_sample(self._h, C.byref(cp), _ptr(lists), _ptr(points), N, _ptr(out), fmt, _ptr(am),
                                                   self._stream()))
        return (out, am) if want_argmax else out

    def render_view(self, params, lists, axes, batches, out=None, dtype=torch.float32, want_argmax=False):
        """Viewport decode (include/smoe_hip.h: smoe_shared_render_view): the dense view ``[*E, C]`` whose axis ``l`` has the
        ``E_l`` coordinates ``axes[l]`` (float32 device table, image units) and is evaluated with the lists of the batches
        ``batches[l]`` (int32 device table ``[E_l]`` of batch indices on that axis, ``0 .. grid_l - 1``).  ``lists`` as in
        ``sample``.  Returns the image, with ``want_argmax`` also the int32 global kernel ids ``[*E]`` (-1: none)."""
        who = "render_view"
        extent = self._check_view(who, dtype, axes, batches, lists)
        out, fmt, am = self._dense_planes(who, extent, out, dtype, want_argmax)
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_shared_render_view(self._h, C.byref(cp), _ptr(lists), _slots(C.c_int32, extent, 1),
                                                    self._axis_slots(axes), self._axis_slots(batches), _ptr(out), fmt, _ptr(am),
                                                    self._stream()))
        return (out, am) if want_argmax else out

    def _check_points(self, who, points, lists):
        """``points`` and ``lists`` as the point decoders take them; returns N."""
        d = self.cfg.dim
        if points.dim() != 2 or points.shape[1] != d or points.dtype != torch.float32 or not points.is_contiguous() \
                or points.device != self.device:
            raise ValueError(f"{who}: points must be a contiguous float32 tensor [N, {d}] on {self.device}")
        self._check_all_lists(who, lists)
        return int(points.shape[0])

    def _check_view(self, who, dtype, axes, batches, lists):
        """The tables and ``lists`` as the viewport decoders take them; returns the extent."""
        self._check_render_arity(who, dtype, axes, (batches,), "axes and batches")
        self._check_axis_tables(who, axes)
        extent = [int(t.numel()) for t in axes]
        for l, t in enumerate(batches):
            if t.dim() != 1 or t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device \
                    or t.numel() != extent[l]:
                raise ValueError(f"{who}: every batch table must be a contiguous 1-d int32 tensor on {self.device} "
                                 f"with as many entries as its axis table ({extent})")
        self._check_all_lists(who, lists)
        return extent

    def _grad_planes(self, who, shape, out, want_values, want_batch):
        """The Jacobian plane ``[*shape, d, C]`` (``out`` checked, or a new one), the value plane and the batch plane or None."""
        full = tuple(shape) + (self.cfg.dim, self.cfg.channels)
        if out is None:
            out = torch.empty(full, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != full or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"{who}: out must be a contiguous float32 tensor {full} on {self.device}")
        val = torch.empty(tuple(shape) + (self.cfg.channels,), dtype=torch.float32, device=self.device) if want_values else None
        bk = torch.empty(tuple(shape), dtype=torch.int32, device=self.device) if want_batch else None
        return out, val, bk

    def sample_grad(self, params, lists, points, out=None, want_values=False, want_batch=False):
        """Point derivative (include/smoe_hip.h: smoe_shared_sample_grad): the exact spatial derivative of the model at
        ``sample``'s points, with ``sample``'s lists, into ``[N, d, C]`` float32: ``jac[i, l, c] = dv_c / dx_l`` per source
        pixel, of the value before the lattice.  Points outside the image give 0.  Returns the Jacobian, then with
        ``want_values`` the float32 values before the lattice ``[N, C]`` and with ``want_batch`` the int32 global ids of the
        owning batches ``[N]`` (-1: outside)."""
        who = "sample_grad"
        N = self._check_points(who, points, lists)
        out, val, bk = self._grad_planes(who, (N,), out, want_values, want_batch)
        if N > 0:
            cp = self._cparams(params)
            _lib.check(self.lib.smoe_shared_sample_grad(self._h, C.byref(cp), _ptr(lists), _ptr(points), N, _ptr(out), _ptr(val),
                                                        _ptr(bk), self._stream()))
        res = (out,) + ((val,) if want_values else ()) + ((bk,) if want_batch else ())
        return res if len(res) > 1 else out

    def sample_area(self, params, lists, points, footprint, taps, out=None, dtype=torch.float32, want_mean=False,
                    want_count=False, want_batch=False):
        """Anti-aliased point decode (include/smoe_hip.h: smoe_shared_sample_area): per point -- the centre of an output cell,
        as ``sample``'s points -- the mean of the model over a regular grid of ``taps[m]`` taps along view axis ``m`` inside
        the cell's ``footprint`` (host ``[d, d]``, column ``m`` = the cell's edge vector along view axis ``m`` in source
        pixels; ``blocks.area_taps`` states the positions), every tap with the kernel list of the batch that owns it, put on
        the lattice, into ``[N, C]``.  Taps outside the image are left out of the mean.  ``lists`` as in ``sample``.  Returns
        the lattice values, then with ``want_mean`` the float32 means before the lattice ``[N, C]``, with ``want_count`` the
        uint8 number of taps inside ``[N]`` and with ``want_batch`` the int32 global id of the batch that owns the centre
        ``[N]`` (-1: outside)."""
        who = "sample_area"
        N = self._check_points(who, points, lists)
        d = self.cfg.dim
        try:
            F, tp = blk.area_args(footprint, taps, d)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        out, fmt, _ = self._dense_planes(who, (N,), out, dtype, False)
        mean = torch.empty((N, self.cfg.channels), dtype=torch.float32, device=self.device) if want_mean else None
        cnt = torch.empty((N,), dtype=torch.uint8, device=self.device) if want_count else None
        bk = torch.empty((N,), dtype=torch.int32, device=self.device) if want_batch else None
        if N > 0:
            cp = self._cparams(params)
            _lib.check(self.lib.smoe_shared_sample_area(self._h, C.byref(cp), _ptr(lists), _ptr(points), N,
                                                        (C.c_float * (d * d))(*[float(v) for v in F.reshape(-1)]),
                                                        (C.c_int32 * d)(*tp), _ptr(out), fmt, _ptr(mean), _ptr(cnt), _ptr(bk),
                                                        self._stream()))
        res = (out,) + ((mean,) if want_mean else ()) + ((cnt,) if want_count else ()) + ((bk,) if want_batch else ())
        return res if len(res) > 1 else out

    def sample_area_each(self, params, lists, points, footprints, taps, out=None, dtype=torch.float32, want_mean=False,
                         want_count=False, want_batch=False):
        """Anti-aliased point decode with a footprint of its own per point (include/smoe_hip.h:
        smoe_shared_sample_area_each): ``sample_area`` where point ``i`` has the footprint ``footprints[i]`` and the tap counts
        ``taps[i]`` -- contiguous device tensors, float32 ``[N, d, d]`` and uint8 ``[N, d]`` (``blocks.area_taps_each`` states
        the positions).  A point whose taps are outside 1 .. 16, multiply to more than 64 or whose footprint is not finite is
        void: 0 / 0 / count 0.  Everything else, and what is returned, is ``sample_area``'s."""
        who = "sample_area_each"
        N = self._check_points(who, points, lists)
        d = self.cfg.dim
        if not torch.is_tensor(footprints) or tuple(footprints.shape) != (N, d, d) or footprints.dtype != torch.float32 \
                or not footprints.is_contiguous() or footprints.device != self.device:
            raise ValueError(f"{who}: footprints must be a contiguous float32 tensor [{N}, {d}, {d}] on {self.device}")
        if not torch.is_tensor(taps) or tuple(taps.shape) != (N, d) or taps.dtype != torch.uint8 or not taps.is_contiguous() \
                or taps.device != self.device:
            raise ValueError(f"{who}: taps must be a contiguous uint8 tensor [{N}, {d}] on {self.device}")
        out, fmt, _ = self._dense_planes(who, (N,), out, dtype, False)
        mean = torch.empty((N, self.cfg.channels), dtype=torch.float32, device=self.device) if want_mean else None
        cnt = torch.empty((N,), dtype=torch.uint8, device=self.device) if want_count else None
        bk = torch.empty((N,), dtype=torch.int32, device=self.device) if want_batch else None
        if N > 0:
            cp = self._cparams(params)
            _lib.check(self.lib.smoe_shared_sample_area_each(self._h, C.byref(cp), _ptr(lists), _ptr(points), N,
                                                             _ptr(footprints), _ptr(taps), _ptr(out), fmt, _ptr(mean),
                                                             _ptr(cnt), _ptr(bk), self._stream()))
        res = (out,) + ((mean,) if want_mean else ()) + ((cnt,) if want_count else ()) + ((bk,) if want_batch else ())
        return res if len(res) > 1 else out

    def render_view_grad(self, params, lists, axes, batches, out=None, want_values=False, want_batch=False):
        """Viewport derivative (include/smoe_hip.h: smoe_shared_render_view_grad): ``sample_grad`` on the dense view of
        ``render_view``'s tables, ``[*E, d, C]``; the other planes ``[*E, C]`` and ``[*E]``."""
        who = "render_view_grad"
        extent = self._check_view(who, torch.float32, axes, batches, lists)
        out, val, bk = self._grad_planes(who, extent, out, want_values, want_batch)
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_shared_render_view_grad(self._h, C.byref(cp), _ptr(lists), _slots(C.c_int32, extent, 1),
                                                         self._axis_slots(axes), self._axis_slots(batches), _ptr(out), _ptr(val),
                                                         _ptr(bk), self._stream()))
        res = (out,) + ((val,) if want_values else ()) + ((bk,) if want_batch else ())
        return res if len(res) > 1 else out

    def accumulate(self, target, params, lists, first_batch=0, loss_out=None, sse_out=None):
        nb = lists.shape[0]
        self._check_target(target, nb)
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_shared_accumulate(self._h, first_batch, nb, _ptr(target), C.byref(cp), _ptr(loss_out),
                                                   _ptr(sse_out), _ptr(lists), self._stream()))

    def apply(self, params, state: AdamState):
        state.c.m = self._cparams(state.m)
        state.c.v = self._cparams(state.v)
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_shared_apply(self._h, C.byref(cp), C.byref(state.c), self._stream()))

    def discard_gradients(self):
        """zero_op alone (smoe.py:1613): drop what accumulate() has gathered since the last apply()."""
        _lib.check(self.lib.smoe_shared_discard(self._h, self._stream()))

    def fit(self, target, params, state: AdamState, lists, n_iters, loss_out=None, sse_out=None):
        self._check_target(target, self.num_batches)
        state.c.m = self._cparams(state.m)
        state.c.v = self._cparams(state.v)
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_shared_fit(self._h, _ptr(target), C.byref(cp), C.byref(state.c), int(n_iters),
                                            _ptr(loss_out), _ptr(sse_out), _ptr(lists), self._stream()))

    def update_kernel_list(self, params, lists, first_batch=0):
        cp = self._cparams(params)
        _lib.check(self.lib.smoe_shared_update_kernel_list(self._h, first_batch, lists.shape[0], C.byref(cp), _ptr(lists),
                                                           self._stream()))

    def set_loss_weights(self, loss_w: Optional[torch.Tensor]):
        """[num_batches, Nb] float32 device tensor of per-pixel loss weights for the WHOLE image (or None to clear);
        the engine keeps a reference so the memory stays alive."""
        if loss_w is not None:
            assert loss_w.dtype == torch.float32 and loss_w.is_contiguous() and loss_w.device == self.device
            assert tuple(loss_w.shape) == (self.num_batches, self.batch_pixels)
        self._loss_w = loss_w
        _lib.check(self.lib.smoe_shared_set_loss_weights(self._h, _ptr(loss_w)))

    def set_center_grid(self, grid: Optional[torch.Tensor]):
        """use_diff_center with quantization_mode 2 / 3: the kernel-grid centres [K, d] (float32, on the device) the trained
        offsets are relative to, or None to clear.  The engine keeps a reference."""
        if grid is not None:
            assert grid.dtype == torch.float32 and grid.is_contiguous() and grid.device == self.device
            assert tuple(grid.shape) == (self.cfg.kernels, len(self.cfg.image_shape))
        self._center_grid = grid
        _lib.check(self.lib.smoe_shared_set_center_grid(self._h, _ptr(grid)))

    def grad_buffer(self) -> torch.Tensor:
        """The gradient accumulation buffer as a float64 device tensor view (for the all-reduce
        between accumulate() and apply() when batches are sharded over ranks)."""
        ptr, cnt = C.c_void_p(), C.c_int64()
        _lib.check(self.lib.smoe_shared_grad_buffer(self._h, C.byref(ptr), C.byref(cnt)))
        n = int(cnt.value)

        class _Arr:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(ptr.value), False), "version": 2}
        return torch.as_tensor(_Arr(), device=self.device)

