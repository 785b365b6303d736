"""``Smoe`` -- host-side mirror of the reference's model facade (reference smoe.py:37-2578)
for the per-block hot path, backed by the HIP kernels in libsmoe_hip.so.

Same entry points, argument names and parameter-dict layout as the reference
(``Smoe(image, kernels_per_dim, ...)``, ``set_optimizer``, ``train``, ``run_batched``,
``get_params`` / ``get_best_params``, ``get_reconstruction`` ...), with block-independent
semantics: ``batch_size`` is the block shape, ``kernels_per_dim`` the kernels per block per
axis, and every block is its own model (own [0,1]^d domain, own K kernels, own Adam state) --
``get_params()[name][b]`` is what the reference's ``Smoe(block_b, ...).get_params()[name]``
returns.  All blocks are fitted by ONE kernel launch per chunk of iterations instead of one
``session.run`` per block per iteration (smoe.py:1643-1702).

Also built: the shared-kernel image mode with batch overlap (``SharedSmoe``), the SSIM loss
(2-d blocks), the parameter quantiser and quantisation-aware fitting (``quantization_mode`` 1-3, ``quantize_pis``),
``train_inverse_cov``, ``radial_as``, ``use_diff_center``, pixel sub-sampling (``sampling_percentage``).  Any kernel grid
is accepted: a kernel count without its own kernel instantiation is padded to the next instantiated one with prior-zero
kernels, which the graph drops (``bool_mask = kernel_list & pis > 0``, smoe.py:480,738).  Not rebuilt (SURVEY section 2
"OUT OF SCOPE"): support vectors, motion models, kernel adding; passing those options raises NotImplementedError
instead of silently doing something else.

Partition invariance: the engine is told the block count of the WHOLE image (``set_total_blocks``), so a rank that
holds a shard of the blocks runs the kernels the whole image would run and every block's result is bit-identical for
any number of ranks -- the reference has one host loop over all blocks (smoe.py:1643-1702).
"""
from __future__ import annotations

import pickle
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import blocks as blk
from . import dist as sdist
from .engine import PARAM_NAMES, EngineConfig, SharedConfig


class Adam:
    """Optimizer configuration object standing in for ``tf.train.AdamOptimizer`` (the
    reference only reads ``_lr`` before handing the object to TF, smoe.py:1120-1144)."""

    def __init__(self, learning_rate: float = 0.001, beta1: float = 0.9, beta2: float = 0.999,
                 epsilon: float = 1e-8):
        self._lr = float(learning_rate)
        self._beta1 = float(beta1)
        self._beta2 = float(beta2)
        self._epsilon = float(epsilon)


def _default_engine_factory(cfg: EngineConfig, device):
    from .engine import BlockEngine          # loads libsmoe_hip.so; fails loudly if absent
    return BlockEngine(cfg, device)


def _default_padded_kernels(dim: int, channels: int, kernels: int, need_full: bool = False) -> int:
    """Smallest instantiated kernel count >= kernels (include/smoe_hip.h: smoe_padded_kernels); need_full: among the
    triples built with the SSIM / quantization_mode 2, 3 kernels (smoe_padded_kernels_full)."""
    from . import _lib
    lib = _lib.load()
    kp = int(lib.smoe_padded_kernels_full(dim, channels, kernels) if need_full else lib.smoe_padded_kernels(dim, channels, kernels))
    if kp < 0:
        raise NotImplementedError(f"no per-block kernel is instantiated for {kernels} or more kernels per block with "
                                  f"(dim={dim}, channels={channels}{', every graph variant' if need_full else ''}); "
                                  "add the triple to csrc/smoe_variants.def")
    return kp


def _pad_kernels(p: Dict[str, np.ndarray], kp: int) -> Dict[str, np.ndarray]:
    """Pad every block's parameter set to kp kernels with kernels that are not part of the graph: prior 0 (smoe.py:480,738:
    bool_mask = kernel_list & pis > 0), centre 0.5, steering identity (any finite value: it is never used)."""
    k = p["pis"].shape[1]
    if kp == k:
        return p
    out = {}
    for name, v in p.items():
        pad = np.zeros((v.shape[0], kp - k) + v.shape[2:], dtype=np.float32)
        if name == "musX":
            pad[...] = 0.5
        elif name == "A_diagonal":
            pad[...] = np.eye(v.shape[-1], dtype=np.float32)
        out[name] = np.ascontiguousarray(np.concatenate([v, pad], axis=1))
    return out


def _fake_quant_fixed(x: torch.Tensor, lb: float, ub: float, bits: int) -> torch.Tensor:
    """tf.quantization.fake_quant_with_min_max_args in fp32 (TF Nudge(): the zero point is rounded so that 0 stays
    representable), for host-side bookkeeping only -- the fit itself quantises inside the kernels."""
    f = torch.float32
    levels = torch.tensor(float(2 ** bits - 1), dtype=f)
    mn, mx = torch.tensor(float(lb), dtype=f), torch.tensor(float(ub), dtype=f)
    scale = (mx - mn) / levels
    zp = -mn / scale
    nzp = torch.clamp(torch.sign(zp) * torch.floor(zp.abs() + 0.5), 0.0, float(levels))
    nmin, nmax = (0.0 - nzp) * scale, (levels - nzp) * scale
    cl = torch.minimum(torch.maximum(x.to(f), nmin.to(x.device)), nmax.to(x.device))
    return torch.floor((cl - nmin.to(x.device)) * (1.0 / scale).to(x.device) + 0.5) * scale.to(x.device) + nmin.to(x.device)


def _warp_chain(jac: torch.Tensor, matrix, d: int) -> torch.Tensor:
    """The chain rule through ``x = M (i + 0.5) + t`` of an affine view, on ``jac``'s device: per output cell
    ``J_view[..., m, c] = sum_l J[..., l, c] M[l, m]`` from the Jacobian per source pixel."""
    M = torch.from_numpy(np.ascontiguousarray(np.asarray(matrix, dtype=np.float64)[:, :d], dtype=np.float32)).to(jac.device)
    return torch.einsum("...lc,lm->...mc", jac, M).contiguous()


def footprint_taps_each_torch(foot: torch.Tensor) -> torch.Tensor:
    """``blocks.footprint_taps_each`` on the device of ``foot`` (float32 ``[N, d, d]``): the same integers -- ceil, max and the
    comparisons are exact in float32 --, uint8 ``[N, d]``."""
    fin = torch.isfinite(foot).all(dim=2).all(dim=1)
    a = torch.where(fin[:, None, None], foot, torch.zeros_like(foot)).abs().amax(dim=1)
    tp = torch.ceil(a).clamp(1, blk.AREA_AXIS_TAPS).to(torch.int64)
    # a fixed number of masked rounds, no read-back: from (16, .., 16) the product is at most 64 after d * 15 decrements at the
    # latest (every count at 1), and a round changes nothing once it is
    for _ in range(tp.shape[1] * (blk.AREA_AXIS_TAPS - 1)):
        over = tp.prod(dim=1) > blk.AREA_TAPS
        ismax = tp == tp.amax(dim=1, keepdim=True)
        first = ismax & (ismax.to(torch.int64).cumsum(dim=1) == 1)                       # the first of equals
        tp = tp - (first & over[:, None]).to(torch.int64)
    return torch.where(fin[:, None], tp, torch.zeros_like(tp)).to(torch.uint8).contiguous()


def map_footprints_torch(p: torch.Tensor) -> torch.Tensor:
    """``blocks.map_footprints`` on the device of ``p`` (float32 ``[*size, d]``): the same float32 differences,
    ``[*size, d, d]``."""
    d = p.shape[-1]
    F = torch.zeros(tuple(p.shape) + (d,), dtype=torch.float32, device=p.device)
    for m in range(d):
        if p.shape[m] < 2:
            continue
        q = p.movedim(m, 0)
        col = torch.empty_like(q)
        col[1:-1] = (q[2:] - q[:-2]) * 0.5
        col[0] = q[1] - q[0]
        col[-1] = q[-1] - q[-2]
        F[..., m] = col.movedim(0, m)
    return F


def _train_loop(m, num_iter, val_iter, ukl_iter, pis_l1, u_l1, callbacks, chunk_limit=None):
    """The iteration / validation / stop logic of ``Smoe.train`` (smoe.py:1485-1603), shared by both facades.  ``m`` supplies
    ``run_batched`` and four hooks: ``_quantize`` (quantize_params [+ rescaler], smoe.py:1498-1505,1539-1545),
    ``_fit_iterations(n)`` (n training passes), ``_readmit_kernels`` (update_kernel_list, smoe.py:1531-1536) and
    ``_keep_best(loss)`` (best snapshot, smoe.py:1574-1576).  The iterations up to the next validation / kernel-list boundary
    run as ONE engine call (``chunk_limit`` = 1 for a fresh pixel draw per pass)."""
    if m.quantization_mode >= 1:                                      # smoe.py:1498-1499
        m._quantize()
    if m.quantization_mode == 1:                                      # smoe.py:1500-1505
        m.best_qloss, m.best_qmse, _, _ = m.run_batched(
            pis_l1=pis_l1, u_l1=u_l1, train=False, update_reconstruction=True, with_quantized_params=True)
        m.qlosses.append((0, m.best_qloss))
        m.qmses.append((0, m.best_qmse))
    # iteration-0 evaluation (smoe.py:1507-1519)
    m.best_loss, m.best_mse, num_pi, num_sv = m.run_batched(pis_l1=pis_l1, u_l1=u_l1, train=False, update_reconstruction=True)
    m._after_first_evaluation()
    m.losses.append((m.iter, m.best_loss))
    m.mses.append((m.iter, m.best_mse))
    m.num_pis.append((m.iter, num_pi))
    m.num_svs.append((m.iter, num_sv))
    for callback in callbacks:
        callback(m)

    loss_val, mse_val = m.best_loss, m.best_mse
    i = 0
    try:
        while i < num_iter:
            # run up to the next validation / kernel-list boundary in ONE launch
            nxt = min(num_iter, (i // val_iter + 1) * val_iter, (i // ukl_iter + 1) * ukl_iter)
            if chunk_limit:
                nxt = min(nxt, i + chunk_limit)
            n = nxt - i
            m._fit_iterations(n)
            i = nxt
            m.iter += n
            m.valid = False
            validate = i % val_iter == 0
            if i % ukl_iter == 0:                                         # smoe.py:1531-1536
                m._readmit_kernels()
                if not validate:
                    loss_val, mse_val, num_pi, num_sv = m.run_batched(pis_l1=pis_l1, u_l1=u_l1, train=False)
            if validate:                                                  # smoe.py:1538-1594
                if m.quantization_mode >= 1:                              # smoe.py:1539-1540
                    m._quantize()
                if m.quantization_mode == 1:                              # smoe.py:1541-1545,1585-1587
                    qloss_val, qmse_val, _, _ = m.run_batched(
                        pis_l1=pis_l1, u_l1=u_l1, train=False, update_reconstruction=True, with_quantized_params=True)
                    m.qlosses.append((i, qloss_val))
                    m.qmses.append((i, qmse_val))
                loss_val, mse_val, num_pi, num_sv = m.run_batched(
                    pis_l1=pis_l1, u_l1=u_l1, train=False, update_reconstruction=True)
                # global divergence rule at validation cadence (per block it is applied on the device every iteration,
                # smoe.py:1565-1570)
                if np.isnan(loss_val) or (len(m.losses) > 0 and loss_val + 1 > (m.losses[0][1] + 100) * 10):
                    print("stop")
                    break
                m._keep_best(loss_val)
                m.losses.append((m.iter, loss_val))
                if not m.best_mse or mse_val < m.best_mse:
                    m.best_mse = mse_val
                m.mses.append((m.iter, mse_val))
                m.num_pis.append((m.iter, num_pi))
                m.num_svs.append((m.iter, num_sv))
                for callback in callbacks:
                    callback(m)
    except KeyboardInterrupt:
        pass
    m.losses_history.append(m.losses)
    m.mses_history.append(m.mses)
    if m.rank == 0:
        print("end loss/mse: ", loss_val, "/", mse_val, "@iter: ", i)
        print("best loss/mse: ", m.best_loss, "/", m.best_mse)


class _SmoeBase:
    """What the two facades share: the optimizer and engine bookkeeping, the getters and ``render``.  A mode supplies
    ``run_batched``, the hooks of ``_train_loop`` and the hooks named below."""
    _unit = None                    # "block" / "batch": what the mode calls a tile of the image in its messages
    _block_local_ids = False        # the engine's render() numbers the kernels per tile, 255 = none (else globally, -1)

    # -- constructor pieces -------------------------------------------------------------------
    def _set_quantizer(self, quantization_mode, quantize_pis, bit_depths, lower_bounds, upper_bounds):
        if quantization_mode not in (0, 1, 2, 3):
            raise ValueError("quantization_mode must be 0, 1, 2 or 3")                # smoe_test.py:298-301
        self.quantization_mode = int(quantization_mode)
        self.quantize_pis = bool(quantize_pis) or quantization_mode >= 2               # smoe_test.py:36-37, smoe.py:474
        # bit depths / bounds in the order A, musX, nu_e, pis, gamma_e; None -> the CLI defaults (smoe_test.py:302-309)
        self.bit_depths = [20, 18, 6, 10, 10] if bit_depths is None else list(bit_depths)
        self.lower_bounds = [-2500, -.3, -5, 0, -32] if lower_bounds is None else list(lower_bounds)
        self.upper_bounds = [2500, 1.3, 5, 2, 32] if upper_bounds is None else list(upper_bounds)

    def _set_image(self, image, precision, margin, use_yuv, only_y_gamma):
        self.image = image = np.asarray(image, dtype=np.float32)
        self.dim_domain = image.ndim - 1                                # smoe.py:227
        self.num_pixel = int(np.prod(image.shape[:self.dim_domain]))    # smoe.py:228
        self.channels = image.shape[-1]
        self.precision, self.margin = precision, margin
        self.use_yuv = bool(use_yuv) and image.shape[-1] == 3           # smoe_test.py:41-44
        self.only_y_gamma = bool(only_y_gamma) and self.use_yuv         # smoe_test.py:43-44, smoe.py:725-729
        return image

    def _batch_shape(self, batch_size, start_batches):
        """smoe.py:231-247: the tile shape from ``batch_size``, or from the desired number of batches (1 -> the image)."""
        image, d = self.image, self.dim_domain
        if batch_size is None or batch_size[0] is None:
            return blk.get_batch_shape(start_batches, tuple(image.shape[:d]) + (d + image.shape[-1],))[:-1]   # smoe.py:229,243
        if len(batch_size) == d:
            return tuple(int(b) for b in batch_size)
        if len(batch_size) == 1:
            return tuple(int(batch_size[0]) for _ in range(d))
        raise ValueError("Required BatchSize doesn't fit to input dimension")    # smoe.py:237

    def _reset_histories(self, iter_offset):
        """smoe.py:183-199."""
        self.losses, self.mses, self.num_pis, self.num_svs = [], [], [], []
        self.qlosses, self.qmses = [], []
        self.losses_history, self.mses_history = [], []
        self.best_loss, self.best_mse = None, []
        self.best_qloss, self.best_qmse = None, []
        self.iter = iter_offset
        self.valid = self.qvalid = False

    # -- engine ---------------------------------------------------------------------------------
    def _start_engine(self, engine_factory, device):
        """The first engine (no optimizer yet); returns its device."""
        self._engine_factory, self._device = engine_factory, device
        self._engine = self._engine_key = None
        self.optimizer1 = self.optimizer2 = self.optimizer3 = None
        self.grad_clip_value_abs = None
        self._make_engine(0.0, 0.0)
        return self._engine.device

    def _make_engine(self, pis_l1: float, u_l1: float):
        """(Re-)create the engine when its configuration changed; ``_config`` adds the mode's shapes to the common
        keywords, ``_engine_created`` hands a fresh engine what it has to know beyond the configuration."""
        o1, o2, o3 = self.optimizer1, self.optimizer2, self.optimizer3
        cfg = self._config(
            channels=self.channels, kernels=self._kp, precision=self.precision, margin=self.margin,
            use_determinant=bool(self.use_determinant), use_yuv=bool(self.use_yuv), train_pis=bool(self.train_pis),
            train_gammas=bool(self.train_gammas), train_musx=bool(self.train_musx),
            lr_expert=o1._lr if o1 else 0.0, lr_pis=o2._lr if o2 else 0.0, lr_steer=o3._lr if o3 else 0.0,
            beta1=o1._beta1 if o1 else 0.9, beta2=o1._beta2 if o1 else 0.999, adam_eps=o1._epsilon if o1 else 1e-8,
            grad_clip=float(self.grad_clip_value_abs or 0.0), pis_l1=float(pis_l1), u_l1=float(u_l1),
            start_pis=self.kernels, only_y_gamma=bool(self.only_y_gamma), ssim_opt=bool(self.ssim_opt),
            quantization_mode=int(self.quantization_mode), quantize_pis=bool(self.quantize_pis),
            bit_depths=tuple(self.bit_depths), lower_bounds=tuple(self.lower_bounds),
            upper_bounds=tuple(self.upper_bounds), train_inverse_cov=bool(self.train_inverse_cov),
            radial_as=bool(self.radial_as), kernel_count_as_norm_l1=self.kernel_count_as_norm_l1)
        key = repr(sorted(cfg.__dict__.items()))
        if key != self._engine_key:
            if self._engine is not None:
                self._engine.close()
            self._engine = self._engine_factory(cfg, self._device)
            self._engine_key = key
            self._engine_created()

    def _hand_over_center_grid(self):
        """use_diff_center with quantization_mode 2 / 3: the graph quantises the OFFSETS (smoe.py:746-747), so the engine
        needs the kernel grid its ``musX`` (= grid + offset) is relative to."""
        if self._mus_grid is None or int(self.quantization_mode) < 2:
            return
        self._mus_grid_dev = torch.from_numpy(np.ascontiguousarray(self._mus_grid, dtype=np.float32)).to(self._engine.device)
        self._engine.set_center_grid(self._mus_grid_dev)

    # -- optimizer (smoe.py:1079-1204) ----------------------------------------------------
    def set_optimizer(self, optimizer1, optimizer2=None, optimizer3=None, optimizer4=None, optimizer5=None,
                      grad_clip_value_abs=None):
        self.optimizer1 = optimizer1
        self.optimizer2 = optimizer1 if optimizer2 is None else optimizer2
        self.optimizer3 = optimizer1 if optimizer3 is None else optimizer3
        self.grad_clip_value_abs = grad_clip_value_abs
        # a fresh set of optimizers means fresh slots and beta powers, as in TF
        self._make_engine(0.0, 0.0)
        self._state = self._engine.new_adam_state(self._params)

    def _begin_train(self, val_iter, ukl_iter, optimizer1, optimizer2, optimizer3, grad_clip_value_abs):
        """The head of ``train`` (smoe.py:1485-1497); returns ``ukl_iter``."""
        if optimizer1:
            self.set_optimizer(optimizer1, optimizer2, optimizer3, grad_clip_value_abs=grad_clip_value_abs)
        assert self.optimizer1 is not None, "no optimizer found, you have to specify one!"
        return val_iter if ukl_iter is None else ukl_iter

    def _count_pis(self) -> torch.Tensor:
        """num_pi_op of the local parameters: it counts pis_mask = qpis > 0 (smoe.py:480,1012)."""
        pis = self._params["pis"]
        if self.quantize_pis:
            pis = _fake_quant_fixed(pis, self.lower_bounds[3], self.upper_bounds[3], self.bit_depths[3])
        return (pis > 0).sum()

    def _quantized_params(self) -> Dict[str, torch.Tensor]:
        """``rparams`` on the device, as the engine takes parameters (smoe.py:1688-1689)."""
        assert self.rparams is not None, "quantize_params + rescaler first (smoe.py:1499-1501)"
        return {k: torch.from_numpy(v).to(self._engine.device) for k, v in self._local_rparams().items()}

    # -- decoding on another grid -------------------------------------------------------------
    def _taps_arg(self, who, taps, footprint):
        """``taps`` of ``render_view`` / ``render_warp`` / ``sample_area`` (``SharedSmoe``: ``eval_view`` / ``eval_warp`` /
        ``eval_points_area``) as one int per view axis (``"auto"``: ``blocks.footprint_taps``), or None where there is
        nothing to average: ``taps`` None or all ones."""
        if taps is None:
            return None
        if isinstance(taps, str):
            if taps != "auto":
                raise ValueError(f'{who}: taps must be "auto", a number or one per axis')
            tp = list(blk.footprint_taps(footprint))
        else:
            try:
                _, tp = blk.area_args(footprint, taps, self.dim_domain)
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
        return None if all(v == 1 for v in tp) else tp

    def _taps_each_arg(self, who, taps, foot, lead):
        """``taps`` of ``sample_area_each`` as a contiguous uint8 ``[N, d]`` tensor on the device of ``foot`` (``[N, d, d]``):
        ``"auto"`` (``blocks.footprint_taps_each``; for a tensor on the GPU the same integers are made there); a number, a
        tuple or a list: one count or one per view axis for all points (checked as ``sample_area``'s -- a ``ValueError`` where
        it would raise one --, then broadcast); an integer ``ndarray`` or tensor: one row per point, ``[..., d]`` exactly (a
        count that is not 0 .. 255 becomes 0: void).  The two are told apart by type, never by shape."""
        d = self.dim_domain
        N = foot.shape[0]
        if isinstance(taps, str):
            if taps != "auto":
                raise ValueError(f'{who}: taps must be "auto", a number, one per axis or an array [..., {d}]')
            if foot.is_cuda:
                return footprint_taps_each_torch(foot)
            return torch.from_numpy(blk.footprint_taps_each(foot.numpy()))
        if isinstance(taps, (int, np.integer, tuple, list)) and not isinstance(taps, bool):
            try:
                _, tp = blk.area_args(np.zeros((d, d), np.float32), taps, d)
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
            return torch.tensor(tp, dtype=torch.uint8, device=foot.device).repeat(N, 1)
        tt = taps if torch.is_tensor(taps) else torch.from_numpy(np.ascontiguousarray(np.asarray(taps)))
        if tuple(tt.shape) != lead + (d,) or tt.dtype.is_floating_point or tt.dtype == torch.bool:
            raise ValueError(f"{who}: taps as an array must be integers {lead + (d,)}")
        tt = tt.to(foot.device).reshape(N, d).to(torch.int64)
        return torch.where((tt < 0) | (tt > 255), torch.zeros_like(tt), tt).to(torch.uint8).contiguous()

    def _ones_taps(self, who, taps):
        """True where ``taps`` of a per-point view asks for nothing to average: None, or a number / one per axis, all ones."""
        if taps is None:
            return True
        if not isinstance(taps, (int, np.integer, tuple, list)) or isinstance(taps, bool):
            return False                                   # "auto", or an array / tensor of per-point counts
        return self._taps_arg(who, taps, np.zeros((self.dim_domain, self.dim_domain))) is None

    def _render(self, scale, samples_per_block, dtype, quantized, want_argmax, to_host, use_lists=True, blend=None):
        """``render`` of both modes.  Hooks: ``_local_rparams``, ``_render_lists(quantized)``, ``_render_grid(m)`` ->
        (tile grid, output extent, one sample table per axis), ``_engine_render`` and, with ``_block_local_ids``,
        ``_global_ids``.  ``blend``: None, or the per-axis half-widths (not all zero) for ``_engine_render_blend``."""
        d, n = self.dim_domain, self.batch_size_valued
        if scale is not None and samples_per_block is not None:
            raise ValueError("render: give scale or samples_per_block, not both")
        if samples_per_block is not None:
            spb = list(np.atleast_1d(samples_per_block))
            spb = spb * d if len(spb) == 1 else spb
            if len(spb) != d:
                raise ValueError(f"render: samples_per_block needs one value or {d}")
            m = [int(v) for v in spb]
        else:
            sc = list(np.atleast_1d(1 if scale is None else scale))
            sc = sc * d if len(sc) == 1 else sc
            if len(sc) != d:
                raise ValueError(f"render: scale needs one value or {d}")
            m = [max(1, int(round(float(v) * nl))) for v, nl in zip(sc, n)]
        if min(m) < 1:
            raise ValueError(f"render: at least one sample per {self._unit} and axis")
        npdt = np.dtype(dtype)
        if npdt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError("render: dtype must be float32 or uint8")
        tdt = torch.uint8 if npdt == np.dtype(np.uint8) else torch.float32
        eng = self._engine
        if not hasattr(eng, "render"):
            raise NotImplementedError("this engine has no render()")
        dev, multi = eng.device, self.world_size > 1
        params = self._quantized_params() if quantized else self._params
        lists = self._render_lists(quantized) if use_lists else None
        grid, extent, axes = self._render_grid(m)
        axes = [torch.from_numpy(a).to(dev) for a in axes]
        out = torch.zeros(tuple(extent) + (self.channels,), dtype=tdt, device=dev) if multi else None
        if blend is None:
            res = self._engine_render(params, lists, axes, m, grid, extent, out, tdt, want_argmax)
        else:
            res = self._engine_render_blend(params, lists, axes, grid, extent, out, tdt, want_argmax, blend)
        img, ids = res if want_argmax else (res, None)
        if ids is not None:
            ids = ids.to(torch.int64)
            if multi or self._block_local_ids:
                # the tile index of every position, and whether the tile is one of this rank's
                pos = [torch.arange(extent[l], device=dev) // m[l] for l in range(d)]
                bid = pos[0]
                for l in range(1, d):
                    bid = bid.reshape(bid.shape + (1,)) * grid[l] + pos[l]
                own = (bid >= self.lo) & (bid < self.hi)
                if self._block_local_ids:
                    ids = self._global_ids(ids, bid, own)
                if multi:
                    ids = torch.where(own, ids + 1, torch.zeros_like(ids))
        if multi:
            # the positions of other ranks' tiles are zero here: the sum over ranks is the image (ids shifted by one)
            img = sdist.allreduce_sum_(img if tdt == torch.float32 else img.to(torch.int32)).to(tdt)
            if ids is not None:
                ids = sdist.allreduce_sum_(ids) - 1
        if to_host:
            img = img.cpu().numpy()
            ids = None if ids is None else ids.cpu().numpy()
        return (img, ids) if want_argmax else img

    # -- getters (smoe.py:1795-1888) ------------------------------------------------------------
    def get_reconstruction(self):
        if not self.valid:
            self.run_batched(train=False, update_reconstruction=True)
        return self.reconstruction_image

    def get_qreconstruction(self):
        if not self.qvalid:
            self.run_batched(train=False, update_reconstruction=True, with_quantized_params=True)
        return self.qreconstruction_image

    def get_weight_matrix_argmax(self):
        if not self.valid:
            self.run_batched(train=False, update_reconstruction=True)
        return self.weight_matrix_argmax

    def get_psnr(self) -> float:
        """PSNR of the current reconstruction over the valid pixels (plotter.py:14-15)."""
        rec = self.get_reconstruction()
        mse = float(np.mean((rec.astype(np.float64) - self.image.astype(np.float64)) ** 2))
        return float(-10.0 * np.log10(mse))

    def get_qlosses(self):
        return self.qlosses

    def get_qmses(self):
        return self.qmses

    def get_losses(self):
        return self.losses

    def get_mses(self):
        return self.mses

    def get_num_pis(self):
        return self.num_pis

    def get_num_svs(self):
        return self.num_svs

    def get_best_loss(self):
        return self.best_loss

    def get_best_mse(self):
        return self.best_mse

    def get_losses_history(self):
        return self.losses_history

    def get_mses_history(self):
        return self.mses_history

    def get_iter(self):
        return self.iter

    def get_original_image(self):
        return np.squeeze(self.image)


class Smoe(_SmoeBase):
    _unit, _block_local_ids = "block", True

    def __init__(self, image, kernels_per_dim=None, train_pis=True, init_params=None, start_batches=1,
                 batch_size=None, train_gammas=True, train_musx=True, use_diff_center=False, radial_as=False,
                 use_determinant=False, normalize_pis=True, quantization_mode=0, bit_depths=None,
                 quantize_pis=False, lower_bounds=None, upper_bounds=None, use_yuv=True, only_y_gamma=False,
                 ssim_opt=False, precision=8, add_kernel_slots=0, iter_offset=0, margin=0.5,
                 overlap_of_batches=0, kernel_count_as_norm_l1=False, train_svs=False, affines=None,
                 train_trafo=False, num_params_model=6, train_inverse_cov=True, init_flag=1,
                 only_rec_from_checkpoint=False, loss_mask=None, device=None, engine_factory=None):
        # -- options outside the hot path: refuse loudly ---------------------------------
        unsupported = {

            "train_svs": train_svs, "train_trafo": train_trafo,
        }
        for name, val in unsupported.items():
            if val:
                raise NotImplementedError(f"Smoe({name}=True) is outside the per-block hot path (SURVEY section 8)")
        self._set_quantizer(quantization_mode, quantize_pis, bit_depths, lower_bounds, upper_bounds)
        if add_kernel_slots:
            raise NotImplementedError("progressive kernel adding changes K over time; not part of the hot path")
        if overlap_of_batches:
            raise NotImplementedError("overlapping batches belong to the shared-kernel mode (SURVEY 8(f-1))")
        if affines is not None:
            raise NotImplementedError("per-frame motion models are out of scope")
        assert kernels_per_dim is not None or init_params is not None, \
            "You need to specify the kernel grid size or give initial parameters."   # smoe.py:249-250

        image = self._set_image(image, precision, margin, use_yuv, only_y_gamma)
        self.ssim_opt = ssim_opt
        self.use_diff_center = use_diff_center
        self.radial_as = radial_as
        self.kernel_count_as_norm_l1 = bool(kernel_count_as_norm_l1)
        self.use_determinant = use_determinant
        self.train_pis, self.train_gammas, self.train_musx = train_pis, train_gammas, train_musx
        self.train_inverse_cov = train_inverse_cov
        self.train_trafo = train_trafo
        self.affines = affines
        self.overlap = overlap_of_batches
        self.add_kernel_slots = 0
        self.loss_mask = loss_mask
        self.qparams = None
        self.rparams = None

        # -- block shape (smoe.py:231-247) -----------------------------------------------
        d = self.dim_domain
        bs = self._batch_shape(batch_size, start_batches)
        self.batch_size_valued = bs
        self.batch_size = bs
        self.grid = blk.grid_shape(image.shape[:d], bs)
        self.num_blocks = int(np.prod(self.grid))
        self.start_batches = self.num_blocks                             # smoe.py:247
        self.padded = blk.padded_shape(image.shape[:d], bs) != tuple(image.shape[:d])
        if self.ssim_opt:
            # loss_pixel = 1 - SSIM (smoe.py:929,980-1011).  The reference's SSIM branch ignores the per-pixel loss
            # weights, so neither a loss mask nor the edge-replicated padding of ragged images can be honoured.
            # 3-d blocks: the 11x11x11 window (smoe.py:999-1003), the time axis padded by 5 like the others
            if min(bs) < 5:
                raise ValueError("ssim_opt pads every block SYMMETRIC by 5: blocks need at least 5 pixels per axis")
            if loss_mask is not None or self.padded:
                raise NotImplementedError("ssim_opt ignores loss weights (as the reference does): no loss_mask, and "
                                          "the image must be a multiple of the block shape")

        # -- shard the independent blocks over ranks ------------------------
        self.rank, self.world_size = sdist.world()
        self.lo, self.hi = sdist.shard_range(self.num_blocks, self.rank, self.world_size)
        all_blocks, valid = blk.image_to_blocks(image, bs)
        blocks_local = all_blocks[self.lo:self.hi]
        self.B = blocks_local.shape[0]
        N = int(np.prod(bs))
        self.N = N
        C = self.channels

        # -- initial parameters (smoe.py:252-262) ----------------------------------------
        if init_params:
            p0 = {k: np.asarray(init_params[k], dtype=np.float32) for k in PARAM_NAMES}
            if radial_as and p0["A_diagonal"].ndim == p0["pis"].ndim:        # the reference's (K,) variable (smoe.py:429-433)
                p0["A_diagonal"] = p0["A_diagonal"][..., None, None] * np.eye(d, dtype=np.float32)
            if p0["pis"].ndim == 1:                       # a single block's dict: broadcast
                p0 = {k: np.broadcast_to(v, (self.num_blocks,) + v.shape).copy() for k, v in p0.items()}
            if p0["pis"].shape[0] != self.num_blocks:
                raise ValueError("init_params must carry one parameter set per block")
            p0 = {k: np.ascontiguousarray(v[self.lo:self.hi]) for k, v in p0.items()}
            K = p0["pis"].shape[1]
            self.musX_init = p0["musX"]
        else:
            kpd = list(kernels_per_dim)
            if len(kpd) == 1:
                kpd = kpd * d
            p0 = blk.init_block_params(blocks_local, kpd, normalize_pis, train_inverse_cov)
            K = p0["pis"].shape[1]
            self.musX_init = blk.gen_domain_grid(kpd, d)
        if radial_as:
            # smoe.py:429-434,714-719: ONE steering value per kernel, A_init[:, 0, 0], tiled over the diagonal; A_corr is
            # not trainable.  The engine keeps A_diagonal (B,K,d,d) with equal diagonal entries and ties their gradient.
            a0 = p0["A_diagonal"][:, :, 0, 0]
            p0["A_diagonal"] = np.ascontiguousarray(a0[..., None, None] * np.eye(d, dtype=np.float32))
        self.kernels = K
        # kernel count of the engine: K itself when a kernel is instantiated for it, else the next instantiated count
        pk = getattr(engine_factory, "padded_kernels", None) if engine_factory is not None else _default_padded_kernels
        need_full = bool(ssim_opt) or int(quantization_mode) >= 2      # graphs only the FULL triples are built for
        if pk is None:
            self._kp = K
        elif engine_factory is None:
            self._kp = int(pk(d, C, K, need_full))
        else:
            self._kp = int(pk(d, C, K))
        p0 = _pad_kernels(p0, self._kp)
        # use_diff_center (smoe.py:390-394,746-747): the trained variable is the OFFSET from the kernel
        # grid (initialised to zero); the engine works on grid + offset, the getters subtract the grid.
        self._mus_grid = None
        if use_diff_center:
            self._mus_grid = np.ascontiguousarray(p0["musX"]).copy()
        self.start_pis = K                                               # smoe.py:264, per block
        self.kernel_count = K * self.num_blocks

        # -- device state ---------------------------------------------------------------
        dev = self._start_engine(engine_factory or _default_engine_factory, device)
        self._target = torch.from_numpy(blk.to_planar(blocks_local)).to(dev)
        lw = None
        if self.padded:
            lw = valid[self.lo:self.hi]
        if loss_mask is not None:                                        # smoe.py:1674-1677
            lm, _ = blk.image_to_blocks(np.asarray(loss_mask, dtype=np.float32)[..., None], bs)
            lm = lm.reshape(self.num_blocks, N)[self.lo:self.hi]
            lw = lm if lw is None else lw * lm
        self._use_loss_mask_default = loss_mask is not None
        self._valid = None if not self.padded else torch.from_numpy(np.ascontiguousarray(valid[self.lo:self.hi])).to(dev)
        self._loss_w = None if lw is None else torch.from_numpy(np.ascontiguousarray(lw, dtype=np.float32)).to(dev)
        self._params = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p0.items()}
        self._best = {k: v.clone() for k, v in self._params.items()}      # smoe.py:861-866
        self._state = self._engine.new_adam_state(self._params)
        self._active = torch.full((self.B,), (1 << K) - 1, dtype=torch.int32, device=dev)   # smoe.py:315 (padding kernels unlisted)
        self._diverged = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self._loss0 = None
        self._best_loss_blocks = None
        # per-pixel sampling probabilities of the sub-sampled passes: uniform until the first reconstruction pass replaces
        # them by the error-proportional ones (smoe.py:270-272,906-907,1768-1769)
        self._sampl_prob = torch.full((self.B, N), 1.0 / N, dtype=torch.float32, device=dev)

        self._reset_histories(iter_offset)
        self._images = None                  # reconstruction_image / weight_matrix_argmax / weight_matrix (lazy, see _stitch)
        self._qimages = None                 # their with_quantized_params counterparts

    # ------------------------------------------------------------------------------------
    def _config(self, **common):
        return EngineConfig(block_shape=self.batch_size_valued, **common)

    def _engine_created(self):
        # the kernels (= the summation order inside a block) are chosen for the whole image, not for this rank's shard
        if hasattr(self._engine, "set_total_blocks"):
            self._engine.set_total_blocks(self.num_blocks)
        self._hand_over_center_grid()

    @property
    def kernel_list_per_batch(self) -> List[np.ndarray]:
        """Per-block boolean kernel lists (smoe.py:315,1763-1766), local blocks only."""
        bits = self._active.cpu().numpy().view(np.uint32)
        K = self.kernels
        mask = ((bits[:, None] >> np.arange(K, dtype=np.uint32)[None, :]) & 1).astype(bool)
        return [m for m in mask]

    # -- passes ----------------------------------------------------------------------------
    def _global(self, loss, sse, valid_only=False):
        s = self._engine.reduce_scalars(loss, sse, None)
        s[2] = self._count_pis().to(torch.float64)       # of this rank's blocks: the parameters are sharded
        sdist.allreduce_sum_(s)
        s = s.cpu().numpy()
        total_px = float(self.num_blocks) * self.N
        loss_val = s[0] / total_px                                   # smoe.py:1758
        # smoe.py:1053,1759.  Ragged images (the reference raises, smoe.py:239-241): passes with a reconstruction count the
        # image's own pixels (run_batched); training passes report the SSE over the padded tiling.
        mse_px = float(self.num_pixel) if valid_only else total_px
        mse_val = s[1] / (mse_px * self.channels) * (2 ** self.precision) ** 2
        return float(loss_val), float(mse_val), int(s[2])

    def run_batched(self, pis_l1=0, u_l1=0, sv_l1_sub_l2=0, train=True, update_reconstruction=False,
                    with_quantized_params=False, sampling_percentage=100, with_inc=False, train_inc=False,
                    thr_sv=None, use_loss_mask=False):
        """One pass over every block (smoe.py:1606-1793).  Returns (loss, mse, num_pi, num_sv)."""
        if with_inc or train_inc:
            raise NotImplementedError("kernel adding is out of scope")
        self.valid = False
        self._make_engine(pis_l1, u_l1)
        eng = self._engine
        sub_w = None
        if train and not self.ssim_opt and sampling_percentage < 100:       # smoe.py:1664-1667
            sub_w = self._sample_pixels(sampling_percentage)
        if with_quantized_params:
            # smoe.py:1688-1689: the rescaled parameters are fed over the masked-parameter tensors;
            # the kernel lists are not touched (smoe.py:1763)
            rp = self._quantized_params()
            self.qvalid = False
            out = eng.forward(self._target, rp, self._active, loss_w=self._loss_w,
                              want_recon=update_reconstruction, want_argmax=update_reconstruction,
                              want_gate=update_reconstruction, update_active=False)
            if update_reconstruction:
                self._stitch(out, quantised=True)
            loss_val, mse_val, num_pi = self._global(out["loss"], out["sse"])
            return loss_val, mse_val, num_pi, 0
        if train:
            assert self.optimizer1 is not None, "no optimizer found, you have to specify one!"
            # (zeros, not empty: smoe_fit leaves the entries of the blocks that were frozen before this pass untouched)
            loss = torch.zeros((self.B,), dtype=torch.float32, device=eng.device)
            sse = torch.zeros((self.B,), dtype=torch.float32, device=eng.device)
            eng.fit(self._target, self._params, self._state, self._active, 1,
                    loss_w=self._loss_w if sub_w is None else sub_w,
                    diverged=self._diverged, loss0=self._loss0, loss_out=loss, sse_out=sse,
                    **({} if sub_w is None else {"loss_w_is_sample": True}))
        else:
            if update_reconstruction:
                # the pass evaluates with the kernel lists it starts from and prunes them afterwards: render() of the
                # same state evaluates with these
                self._recon_active = self._active.clone()
            out = eng.forward(self._target, self._params, self._active, loss_w=self._loss_w,
                              want_recon=update_reconstruction, want_argmax=update_reconstruction,
                              want_gate=update_reconstruction)
            loss, sse = out["loss"], out["sse"]
            if update_reconstruction and self._valid is not None:
                # ragged image: the kernels' SSE runs over the edge-replicated padding too; with the reconstruction at
                # hand the reported MSE counts the image's own pixels only (equal to get_psnr() on the cropped image)
                sse = (((out["recon"] - self._target) ** 2) * self._valid[:, None, :]).sum(dim=(1, 2))
            if update_reconstruction:
                self._stitch(out)
                # smoe.py:906-907,1768-1769: per-pixel sampling probabilities of the next sub-sampled passes
                err = ((out["recon"] - self._target) ** 2).mean(dim=1)                  # (B, N)
                self._sampl_prob = err / err.sum(dim=1, keepdim=True).clamp_min(1e-30)
        loss_val, mse_val, num_pi = self._global(loss, sse, valid_only=(not train) and update_reconstruction and self._valid is not None)
        self._last_block_loss = loss
        return loss_val, mse_val, num_pi, 0

    def _sample_pixels(self, sampling_percentage):
        """Pixel sub-sampling (smoe.py:1664-1667): every block trains on round(N * p / 100) pixels drawn without
        replacement with the error-proportional probabilities of the last reconstruction pass (smoe.py:906-907; uniform
        before the first one, smoe.py:270-272).  The
        reference feeds only the drawn pixels; here they get the loss weight N / n (the others 0), which gives the same
        loss and the same gradients -- `mean` over the n drawn pixels.  Draws: exponential-race keys (the successive-
        sampling law of numpy's `choice(replace=False, p=...)`, another random stream).  The engine is told that the weights are
        a sample (``loss_w_is_sample``): pixels that were not drawn do not vote in the kernel-list prune, as in the reference,
        which never sees them.  With a loss mask on top, drawn pixels the mask zeroes do not vote either (the reference
        feeds them with weight 0: they would)."""
        B, N = self._sampl_prob.shape
        n = max(1, int(round(N * sampling_percentage / 100.0)))
        gen = getattr(self, "_sample_gen", None)
        if gen is None:
            gen = self._sample_gen = torch.Generator(device=self._sampl_prob.device)
            gen.manual_seed(20260000 + self.rank)
        u = torch.rand((B, N), generator=gen, device=self._sampl_prob.device, dtype=torch.float32).clamp_min(1e-30)
        keys = -torch.log(u) / self._sampl_prob.clamp_min(1e-12)          # smallest keys win
        idx = torch.topk(keys, n, dim=1, largest=False).indices
        w = torch.zeros((B, N), dtype=torch.float32, device=self._sampl_prob.device)
        w.scatter_(1, idx, float(N) / float(n))
        if self._loss_w is not None:
            w = w * self._loss_w
        return w.contiguous()

    def _assemble_one(self, out, name):
        """One full-image product (reconstruction / argmax / gate) from a pass's device outputs (smoe.py:1719-1783)."""
        bs, d = self.batch_size_valued, self.dim_domain
        if name == "image":
            recon = blk.from_planar(out["recon"].cpu().numpy(), bs)                   # (B,*bs,C)
            recon = sdist.allgather_blocks(recon, self.num_blocks)
            return blk.blocks_to_image(recon, self.image.shape[:d], bs)
        if name == "argmax":
            am = out["argmax"].cpu().numpy().astype(np.int64).reshape((self.B,) + bs)
            am = am + (np.arange(self.lo, self.hi, dtype=np.int64) * self.kernels).reshape((-1,) + (1,) * d)
            am = sdist.allgather_blocks(am, self.num_blocks)
            return blk.blocks_to_image(am[..., None], self.image.shape[:d], bs)[..., 0]
        gate = out["gate_w"].cpu().numpy().reshape((self.B, self._kp) + bs)[:, :self.kernels]
        return sdist.allgather_blocks(gate, self.num_blocks)                          # gate: (B,K,*bs)

    def _assemble(self, out):
        return tuple(self._assemble_one(out, n) for n in ("image", "argmax", "gate"))

    def _stitch(self, out, quantised=False):
        """Keep the products of an update_reconstruction pass.  Single process: the device tensors are kept and the
        host copy + stitching (tens of ms for large images) happens per product when an attribute / getter asks; several ranks:
        assembled right away, because the gather is a collective every rank takes part in."""
        slot = "_qimages" if quantised else "_images"
        if self.world_size == 1:
            setattr(self, slot, {"pending": out})
        else:
            setattr(self, slot, dict(zip(("image", "argmax", "gate"), self._assemble(out))))
        if quantised:
            self.qvalid = True
        else:
            self.valid = True

    def _image_product(self, slot, name):
        st = getattr(self, slot)
        if st is None:
            return None
        if name not in st:                 # single process: each product is copied to the host and stitched when first asked for
            st[name] = self._assemble_one(st["pending"], name)
            if all(n in st for n in ("image", "argmax", "gate")):
                del st["pending"]
        return st[name]

    reconstruction_image = property(lambda self: self._image_product("_images", "image"))
    weight_matrix_argmax = property(lambda self: self._image_product("_images", "argmax"))
    weight_matrix = property(lambda self: self._image_product("_images", "gate"))
    qreconstruction_image = property(lambda self: self._image_product("_qimages", "image"))
    qweight_matrix_argmax = property(lambda self: self._image_product("_qimages", "argmax"))
    qweight_matrix = property(lambda self: self._image_product("_qimages", "gate"))

    # -- training loop (smoe.py:1485-1603) -------------------------------------------------
    def train(self, num_iter, val_iter=100, ukl_iter=None, optimizer1=None, optimizer2=None, optimizer3=None,
              grad_clip_value_abs=None, pis_l1=0, u_l1=0, sv_l1_sub_l2=0, sampling_percentage=100,
              callbacks=(), with_inc=False, train_inc=False, train_orig=True, use_loss_mask=False):
        ukl_iter = self._begin_train(val_iter, ukl_iter, optimizer1, optimizer2, optimizer3, grad_clip_value_abs)
        if with_inc or train_inc or not train_orig:
            raise NotImplementedError("kernel-adding options are outside the hot path")
        self._train_sampling = sampling_percentage if (sampling_percentage < 100 and not self.ssim_opt) else None
        self._make_engine(pis_l1, u_l1)
        _train_loop(self, num_iter, val_iter, ukl_iter, pis_l1, u_l1, callbacks,
                    chunk_limit=1 if self._train_sampling is not None else None)   # a fresh pixel draw per pass (smoe.py:1664-1667)

    # hooks of _train_loop
    def _quantize(self):
        from .quantizer import quantize_params, rescaler
        self.qparams = quantize_params(self, self.get_params())
        if self.quantization_mode == 1:
            self.rparams = rescaler(self, self.qparams)

    def _after_first_evaluation(self):
        if self._loss0 is None:
            self._loss0 = self._last_block_loss.clone()
        if self._best_loss_blocks is None:
            self._best_loss_blocks = self._last_block_loss.clone()
            for k in PARAM_NAMES:
                self._best[k].copy_(self._params[k])

    def _fit_iterations(self, n):
        sp = getattr(self, "_train_sampling", None)
        self._engine.fit(self._target, self._params, self._state, self._active, n,
                         loss_w=self._sample_pixels(sp) if sp is not None else self._loss_w,
                         diverged=self._diverged, loss0=self._loss0,
                         **({} if sp is None else {"loss_w_is_sample": True}))

    def _readmit_kernels(self):
        self._engine.update_kernel_list(self._params, self._active)

    def _keep_best(self, loss_val):
        self._engine.checkpoint_best(self._last_block_loss, self._best_loss_blocks, self._params, self._best)
        if not self.best_loss or loss_val < self.best_loss:
            self.best_loss = loss_val

    # -- getters (smoe.py:1795-1888) ------------------------------------------------------------
    def _gather_params(self, p: Dict[str, torch.Tensor]) -> Dict[str, np.ndarray]:
        out = {k: v.cpu().numpy().copy() for k, v in p.items()}
        if self._mus_grid is not None:                     # use_diff_center: report the trained offsets
            out["musX"] = out["musX"] - self._mus_grid
        out = {k: np.ascontiguousarray(v[:, :self.kernels]) for k, v in out.items()}     # without the padding kernels
        if self.radial_as:                                 # the reference's variable is (K,) per model
            out["A_diagonal"] = np.ascontiguousarray(out["A_diagonal"][:, :, 0, 0])
        return {k: sdist.allgather_blocks(v, self.num_blocks) for k, v in out.items()}

    def get_params(self):
        return self._gather_params(self._params)

    def get_best_params(self):
        return self._gather_params(self._best)

    def render(self, scale=None, samples_per_block=None, dtype=np.float32, quantized=False, want_argmax=False,
               to_host=True, blend=0.0):
        """Decode the fitted blocks on another sampling grid, on the device (the engine's ``render``): every block is a
        continuous function of the coordinate, so zooming, a finer pitch or frames between the fitted ones are "evaluate
        the same model somewhere else" -- no pixel is interpolated.
        ``blend``: a number or one per axis, in source pixels (``0 .. n_l / 2``).  Every block is fitted alone, so the
        stitched function jumps at the block borders -- a grid of seams at 2x or 4x.  With ``blend > 0`` the neighbouring
        block's model is evaluated too within ``blend`` pixels of a border and the two (2^d at a corner) are cross-faded,
        1/2 : 1/2 on the seam (the engine's ``render_blend``; include/smoe_hip.h: smoe_render_blend): one continuous
        function from the same fitted models.  Samples farther than ``blend`` from every border are unchanged, and so is
        the kernel map of ``want_argmax``.  0 (the default) is the plain decoder.
        ``scale``: a number or one per axis, ``m_l = round(scale_l * n_l)`` samples per block (at least 1);
        ``samples_per_block``: the ``m_l`` themselves (a number or one per axis); neither: the training lattice.
        Sample positions: ``blocks.render_axis``.  Output extent ``E_l = image.shape[l] * m_l // n_l`` (the padding of a
        ragged image is cropped), layout ``[*E, C]`` as ``get_reconstruction()``; ``dtype`` float32 (lattice values) or
        uint8 (lattice indices).  ``quantized``: render ``rparams`` (what ``get_qreconstruction`` evaluates).
        ``want_argmax``: also the map of global kernel ids ``[*E]`` (int64, block offset added as in
        ``get_weight_matrix_argmax``; -1 where no kernel has influence on the sample).  ``to_host=False`` returns device
        tensors.  Several ranks: every rank renders its blocks and the images are summed; the result is the same on
        every rank and for every number of ranks."""
        bl = self._blend_arg("render", blend)
        return self._render(scale, samples_per_block, dtype, quantized, want_argmax, to_host, blend=bl)

    def render_view(self, window, size=None, scale=None, dtype=np.float32, quantized=False, want_argmax=False,
                    to_host=True, blend=0.0, taps=None):
        """Decode a viewport: the axis-aligned ``window`` of the image domain at the output ``size``, on the device (the
        engine's ``render_view``; include/smoe_hip.h: smoe_render_view).  Only the window is computed and stored: an 8x
        detail, a fit-to-window zoom of any ratio, a thumbnail with fewer samples than blocks, one frame of a video.
        ``window``: one ``(lo, hi)`` per axis in source pixels (pixel ``q`` covers ``[q, q + 1)``, ``0 <= lo < hi <=
        image.shape[l]``; None for an axis: the whole axis).  ``size``: the ``E_l`` output samples per axis, or ``scale``
        (a number or one per axis): ``E_l = max(1, round((hi - lo) * scale_l))``; not both, neither: scale 1.  Sample
        positions: ``blocks.view_axis`` -- a window that is a crop of a ``render`` grid gives exactly that crop.
        ``dtype``, ``quantized``, ``blend`` and the global ids of ``want_argmax`` (int64, -1: none) are ``render``'s; the
        kernel lists are ``render``'s too.  Returns the image ``[*E, C]``.  Several ranks: parameters and lists are gathered
        and every rank renders the whole view (a view is small); the result is the same on every rank and for every
        number of ranks.
        ``taps``: None (the default) or all ones: one position per sample, as above.  Otherwise (a number, one per axis or
        ``"auto"``) every sample is the mean over ``taps[l]`` taps per axis inside its cell -- ``sample_area`` at the same
        positions ``x_i`` (rounded to float32 once) with the footprint ``diag((hi - lo) / E)``: a thumbnail that does not
        alias.  ``want_argmax`` is refused then (an average has no single kernel)."""
        d, n = self.dim_domain, self.batch_size_valued
        bl = self._blend_arg("render_view", blend)
        window = [None] * d if window is None else list(window)
        if len(window) != d:
            raise ValueError(f"render_view: window needs one (lo, hi) per axis ({d})")
        win = [(0.0, float(self.image.shape[l])) if w is None else (float(w[0]), float(w[1])) for l, w in enumerate(window)]
        for l, (lo, hi) in enumerate(win):
            if not (0.0 <= lo < hi <= float(self.image.shape[l])):
                raise ValueError(f"render_view: window[{l}] must satisfy 0 <= lo < hi <= {int(self.image.shape[l])}")
        if size is not None and scale is not None:
            raise ValueError("render_view: give size or scale, not both")
        if size is not None:
            E = [int(v) for v in np.atleast_1d(size)]
            E = E * d if len(E) == 1 else E
            if len(E) != d or min(E) < 1:
                raise ValueError(f"render_view: size needs {d} entries >= 1")
        else:
            sc = list(np.atleast_1d(1 if scale is None else scale))
            sc = sc * d if len(sc) == 1 else sc
            if len(sc) != d:
                raise ValueError(f"render_view: scale needs one value or {d}")
            E = [max(1, int(round((hi - lo) * float(v)))) for (lo, hi), v in zip(win, sc)]
        npdt = np.dtype(dtype)
        if npdt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError("render_view: dtype must be float32 or uint8")
        tdt = torch.uint8 if npdt == np.dtype(np.uint8) else torch.float32
        foot = np.diag([(hi - lo) / e for (lo, hi), e in zip(win, E)])
        tp = self._taps_arg("render_view", taps, foot)
        if tp is not None:
            if want_argmax:
                raise ValueError("render_view: want_argmax needs taps=None (an average has no single kernel)")
            axes = [blk.view_positions(lo, hi, e) for (lo, hi), e in zip(win, E)]     # view_axis' x_i, rounded once
            pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
            return self.sample_area(pts, foot, taps=tp, dtype=dtype, quantized=quantized, to_host=to_host, blend=blend)
        eng = self._engine
        if not hasattr(eng, "render_view"):
            raise NotImplementedError("this engine has no render_view()")
        dev = eng.device
        tabs = [blk.view_axis(n[l], self.grid[l], self.image.shape[l], win[l][0], win[l][1], E[l]) for l in range(d)]
        params, active, center = self._whole_model(quantized)
        res = eng.render_view(params, active, self.grid, [t[0] for t in tabs], [t[2] for t in tabs],
                              [torch.from_numpy(t[3]).to(dev) for t in tabs], blend=bl,
                              dtype=tdt, want_argmax=want_argmax, center_grid=center)
        img, ids = res if want_argmax else (res, None)
        if ids is not None:
            # the block of every position from the start tables
            pos = [torch.from_numpy(t[0] + np.repeat(np.arange(t[1]), np.diff(t[2]))).to(dev) for t in tabs]
            bid = pos[0]
            for l in range(1, d):
                bid = bid.reshape(bid.shape + (1,)) * self.grid[l] + pos[l]
            ids = self._global_ids(ids.to(torch.int64), bid, torch.ones_like(bid, dtype=torch.bool))
        if to_host:
            img = img.cpu().numpy()
            ids = None if ids is None else ids.cpu().numpy()
        return (img, ids) if want_argmax else img

    def _whole_model(self, quantized):
        """Parameters, kernel lists (``render``'s) and centre grid of ALL blocks on this rank's device, as ``render_view`` and
        ``sample`` hand them to the engine: with several ranks everyone's are gathered (small: a few hundred bytes per block)."""
        dev = self._engine.device
        params = self._quantized_params() if quantized else self._params
        active = self._render_lists(quantized)
        center = None
        if self.world_size > 1:
            full = lambda t: torch.from_numpy(np.ascontiguousarray(sdist.allgather_blocks(t.cpu().numpy(), self.num_blocks))).to(dev)
            params = {k: full(v) for k, v in params.items()}
            active = None if active is None else full(active)
            if self._mus_grid is not None and int(self.quantization_mode) >= 2:
                center = torch.from_numpy(np.ascontiguousarray(sdist.allgather_blocks(self._mus_grid, self.num_blocks),
                                                               dtype=np.float32)).to(dev)
        return params, active, center

    def _blend_arg(self, who, blend):
        """``blend`` of ``render``, ``render_view``, ``sample`` and ``sample_grad`` (a number or one per axis, source pixels,
        ``0 .. n_l / 2``) as the engine takes it: one float per axis, or None where no axis blends."""
        d = self.dim_domain
        bl = [float(v) for v in np.atleast_1d(blend)]
        bl = bl * d if len(bl) == 1 else bl
        if len(bl) != d:
            raise ValueError(f"{who}: blend needs one value or {d}")
        for v, nl in zip(bl, self.batch_size_valued):
            if not np.isfinite(v) or v < 0 or v > nl / 2:
                raise ValueError(f"{who}: blend must lie within 0 .. block size / 2 on every axis")
        return bl if any(v > 0 for v in bl) else None

    def _points_arg(self, who, points, dev):
        """``points`` ``[..., d]`` (array-like or a tensor) as the engine takes them -- a contiguous float32 ``[N, d]`` tensor on
        ``dev`` -- and their leading shape."""
        d = self.dim_domain
        pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points), dtype=np.float32))
        if pts.dim() < 1 or pts.shape[-1] != d:
            raise ValueError(f"{who}: points need a trailing axis of {d} coordinates")
        return pts.to(device=dev, dtype=torch.float32).reshape(-1, d).contiguous(), tuple(pts.shape[:-1])

    def sample(self, points, dtype=np.float32, quantized=False, want_argmax=False, to_host=True, blend=0.0):
        """The model's value at arbitrary positions, on the device (the engine's ``sample``; include/smoe_hip.h: smoe_sample):
        a rotated or warped view, a motion-compensated lookup, a profile along a line, a few thousand probes -- no pixel is
        interpolated.  ``points``: array-like or a device tensor ``[..., d]`` of float32 positions in source pixels, in the
        image's axis order (pixel ``q`` covers ``[q, q + 1)``; ``blocks.point_blocks`` is the mapping).  Returns ``[..., C]``;
        a position outside the image (NaN, ``< 0`` or ``>= image.shape[l]`` on any axis) gives 0.  ``dtype``, ``quantized``,
        ``blend`` and the kernel lists are ``render_view``'s; with ``want_argmax`` also the global kernel ids ``[...]``
        (int64; -1: no kernel has influence, or outside).  The pixel centres ``q + 0.5`` give ``render()`` bit for bit.
        ``to_host=False`` returns device tensors.  Several ranks: parameters and lists are gathered and every rank evaluates
        all points; the result is the same on every rank and for every number of ranks."""
        d = self.dim_domain
        bl = self._blend_arg("sample", blend)
        npdt = np.dtype(dtype)
        if npdt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError("sample: dtype must be float32 or uint8")
        tdt = torch.uint8 if npdt == np.dtype(np.uint8) else torch.float32
        eng = self._engine
        if not hasattr(eng, "sample"):
            raise NotImplementedError("this engine has no sample()")
        dev = eng.device
        pts, lead = self._points_arg("sample", points, dev)
        params, active, center = self._whole_model(quantized)
        res = eng.sample(params, active, self.grid, [int(v) for v in self.image.shape[:d]], pts,
                         blend=bl, dtype=tdt, want_argmax=want_argmax, want_block=want_argmax, center_grid=center)
        img, ids = (res[0], res[1:]) if want_argmax else (res, None)
        img = img.reshape(lead + (self.channels,))
        if ids is not None:
            am, bid = ids[0].to(torch.int64), ids[1].to(torch.int64)
            ids = self._global_ids(am, bid, bid >= 0).reshape(lead)
        if to_host:
            img = img.cpu().numpy()
            ids = None if ids is None else ids.cpu().numpy()
        return (img, ids) if want_argmax else img

    def render_warp(self, matrix, size, taps=None, **options):
        """An affine view of the model: ``sample(blocks.warp_points(matrix, size), **options)``.  ``matrix = [M | t]``
        ``[d, d + 1]`` maps the cell centre ``i + 0.5`` of output index ``i`` to the source position ``M (i + 0.5) + t`` in
        source pixels -- a rotation, a shear, any zoom.  Returns the image ``[*size, C]`` (0 where the view leaves the image);
        ``options`` are ``sample``'s.  ``taps``: None (the default) or all ones: that call.  Otherwise (a number, one per view
        axis or ``"auto"``) ``sample_area`` at the same positions with the footprint ``M`` -- a zoomed-out warp that does not
        alias; ``options`` are ``sample_area``'s then."""
        pts = blk.warp_points(matrix, size)
        M = np.asarray(matrix, dtype=np.float64)[:, :self.dim_domain]
        tp = self._taps_arg("render_warp", taps, M)
        if tp is None:
            return self.sample(pts, **options)
        return self.sample_area(pts, M, taps=tp, **options)

    def sample_area(self, points, footprint, taps="auto", dtype=np.float32, quantized=False, want_mean=False, want_count=False,
                    to_host=True, blend=0.0):
        """Anti-aliased ``sample``, on the device (the engine's ``sample_area``; include/smoe_hip.h: smoe_sample_area): every
        point is the centre of an output cell, and its result is the mean of the model over a regular grid of taps inside the
        cell, put on the lattice -- a decode coarser than the source (a thumbnail, a zoomed-out warp) takes one position per
        cell with ``sample`` and aliases.  ``footprint`` ``[d, d]`` in source pixels: column ``m`` is the edge vector of a cell
        along view axis ``m`` (``M`` of an affine view, ``diag((hi - lo) / E)`` of a viewport); one footprint serves all
        points.  ``taps``: a number, one per view axis (1 .. 16, product at most 64) or ``"auto"``
        (``blocks.footprint_taps``: one tap per source pixel covered).  Positions: ``blocks.area_taps``.  Taps outside the
        image are left out of the mean, so an edge cell stays as bright as an inside one; a cell with no tap inside gives 0.
        ``points``, ``dtype``, ``quantized``, ``blend`` and the kernel lists are ``sample``'s.  Returns ``[..., C]``; with
        ``want_mean`` also the float32 means before the lattice ``[..., C]``, with ``want_count`` the uint8 number of taps
        inside ``[...]``.  ``to_host=False`` returns device tensors.  Several ranks: as ``sample``.  The counterpart for a
        whole-image model is ``SharedSmoe.eval_points_area``."""
        d = self.dim_domain
        bl = self._blend_arg("sample_area", blend)
        npdt = np.dtype(dtype)
        if npdt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError("sample_area: dtype must be float32 or uint8")
        tdt = torch.uint8 if npdt == np.dtype(np.uint8) else torch.float32
        tp = self._taps_arg("sample_area", taps, footprint) or [1] * d
        eng = self._engine
        if not hasattr(eng, "sample_area"):
            raise NotImplementedError("this engine has no sample_area()")
        dev = eng.device
        pts, lead = self._points_arg("sample_area", points, dev)
        params, active, center = self._whole_model(quantized)
        res = eng.sample_area(params, active, self.grid, [int(v) for v in self.image.shape[:d]], pts, footprint, tp,
                              blend=bl, dtype=tdt, want_mean=want_mean, want_count=want_count, center_grid=center)
        res = list(res) if isinstance(res, tuple) else [res]
        res[0] = res[0].reshape(lead + (self.channels,))
        if want_mean:
            res[1] = res[1].reshape(lead + (self.channels,))
        if want_count:
            res[-1] = res[-1].reshape(lead)
        if to_host:
            res = [t.cpu().numpy() for t in res]
        return tuple(res) if len(res) > 1 else res[0]

    def sample_area_each(self, points, footprints, taps="auto", dtype=np.float32, quantized=False, want_mean=False,
                         want_count=False, to_host=True, blend=0.0):
        """``sample_area`` with a footprint of its own for every point, on the device (the engine's ``sample_area_each``;
        include/smoe_hip.h: smoe_sample_area_each) -- a view whose magnification varies across the output: a perspective
        view, a lens or stabilisation map, any dense lookup map.  ``points`` ``[..., d]`` and ``footprints`` ``[..., d, d]``
        (arrays or device tensors; column ``m`` of a footprint is the edge vector of that sample's cell along view axis ``m``,
        source pixels).  ``taps``: ``"auto"`` (``blocks.footprint_taps_each``: one tap per source pixel covered, per point),
        a number or one per view axis (broadcast), or an integer array ``[..., d]``.  Positions: ``blocks.area_taps_each``.
        A point is the result of ``sample_area`` with its footprint and taps, bit for bit.  A point whose taps are outside
        1 .. 16, multiply to more than 64 or whose footprint is not finite is void: 0, mean 0, count 0.  Everything else,
        and what is returned, is ``sample_area``'s."""
        d = self.dim_domain
        who = "sample_area_each"
        bl = self._blend_arg(who, blend)
        npdt = np.dtype(dtype)
        if npdt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError(f"{who}: dtype must be float32 or uint8")
        tdt = torch.uint8 if npdt == np.dtype(np.uint8) else torch.float32
        eng = self._engine
        if not hasattr(eng, "sample_area_each"):
            raise NotImplementedError("this engine has no sample_area_each()")
        dev = eng.device
        pts, lead = self._points_arg(who, points, dev)
        if torch.is_tensor(footprints):
            foot = footprints
        else:
            fa = np.asarray(footprints)
            if fa.dtype.kind not in "fiu":
                raise ValueError(f"{who}: footprints must be numbers")
            foot = torch.from_numpy(np.ascontiguousarray(fa, dtype=np.float32))
        if tuple(foot.shape) != lead + (d, d) or not foot.dtype.is_floating_point:
            raise ValueError(f"{who}: footprints must be floating point {lead + (d, d)}")
        foot = foot.to(device=dev, dtype=torch.float32).reshape(-1, d, d).contiguous()
        tp = self._taps_each_arg(who, taps, foot, lead)
        params, active, center = self._whole_model(quantized)
        res = eng.sample_area_each(params, active, self.grid, [int(v) for v in self.image.shape[:d]], pts, foot, tp,
                                   blend=bl, dtype=tdt, want_mean=want_mean, want_count=want_count, center_grid=center)
        res = list(res) if isinstance(res, tuple) else [res]
        res[0] = res[0].reshape(lead + (self.channels,))
        if want_mean:
            res[1] = res[1].reshape(lead + (self.channels,))
        if want_count:
            res[-1] = res[-1].reshape(lead)
        if to_host:
            res = [t.cpu().numpy() for t in res]
        return tuple(res) if len(res) > 1 else res[0]

    def render_projective(self, H, size, taps="auto", **options):
        """A projective view of the model, anti-aliased: ``sample_area_each`` at ``blocks.projective_points(H, size)``.  ``H``
        ``[d + 1, d + 1]`` maps the cell centre ``c = i + 0.5`` of output index ``i`` to ``(H[:d, :d] c + H[:d, d]) / (H[d, :d] .
        c + H[d, d])`` in source pixels -- a homography; every sample is averaged over its own footprint, the analytic
        Jacobian of the map there.  Returns the image ``[*size, C]``; samples behind the horizon (``s <= 0``) and where the
        view leaves the image give 0.  ``taps``: ``"auto"`` (the default), a number or one per view axis; None or all ones:
        ``sample(points)``.  ``options`` are ``sample_area_each``'s (``sample``'s with ``taps`` None)."""
        try:
            pts, foot, _ = blk.projective_points(H, size)
        except ValueError as e:
            raise ValueError(f"render_projective: {e}") from None
        if self._ones_taps("render_projective", taps):
            return self.sample(pts, **options)
        return self.sample_area_each(pts, foot, taps=taps, **options)

    def render_map(self, points, taps="auto", **options):
        """A dense lookup map of the model, anti-aliased: ``points`` ``[*size, d]`` (an array or a device tensor) holds the
        source position of every output sample -- a lens-distortion or stabilisation map, a fisheye or polar unwrapping --
        and every sample is averaged over its own footprint ``blocks.map_footprints(points)`` (central differences of the map;
        made on the device for a device tensor).  Returns ``[*size, C]``.  ``taps`` and ``options`` as in
        ``render_projective``."""
        d = self.dim_domain
        if (points.dim() if torch.is_tensor(points) else np.ndim(points)) != d + 1 or tuple(points.shape)[-1] != d:
            raise ValueError(f"render_map: points must be [*size, {d}] with {d} view axes")
        if self._ones_taps("render_map", taps):
            return self.sample(points, **options)
        if torch.is_tensor(points):
            if not points.dtype.is_floating_point:
                raise ValueError("render_map: points must be floating point")
            p32 = points.to(torch.float32)
            foot = map_footprints_torch(p32) if p32.is_cuda else torch.from_numpy(blk.map_footprints(p32.numpy()))
            return self.sample_area_each(p32, foot, taps=taps, **options)
        pa = np.asarray(points)
        if pa.dtype.kind not in "fiu":
            raise ValueError("render_map: points must be numbers")
        pa = pa.astype(np.float32)
        return self.sample_area_each(pa, blk.map_footprints(pa), taps=taps, **options)

    def sample_grad(self, points, quantized=False, want_values=False, to_host=True, blend=0.0):
        """The model's exact spatial derivative at arbitrary positions, on the device (the engine's ``sample_grad``;
        include/smoe_hip.h: smoe_sample_grad): an edge map, a structure tensor, the temporal slope of a video model, a
        sub-pixel refinement or alignment step.  Differences of ``sample()`` sit on the 8-bit lattice; this is the closed-form
        derivative of the value before the lattice, with the gate mask and the clip held piecewise constant.  ``points``,
        ``quantized``, ``blend`` and the kernel lists are ``sample``'s.  Returns ``[..., d, C]`` float32,
        ``jac[..., l, c] = dV_c / dx_l`` per source pixel (0 outside the image); with ``want_values`` also the float32
        values before the lattice ``[..., C]``.  ``to_host=False`` returns device tensors.  Several ranks: as ``sample``."""
        d = self.dim_domain
        bl = self._blend_arg("sample_grad", blend)
        eng = self._engine
        if not hasattr(eng, "sample_grad"):
            raise NotImplementedError("this engine has no sample_grad()")
        dev = eng.device
        pts, lead = self._points_arg("sample_grad", points, dev)
        params, active, center = self._whole_model(quantized)
        res = eng.sample_grad(params, active, self.grid, [int(v) for v in self.image.shape[:d]], pts,
                              blend=bl, want_values=want_values, center_grid=center)
        jac, val = res if want_values else (res, None)
        jac = jac.reshape(lead + (d, self.channels))
        if val is not None:
            val = val.reshape(lead + (self.channels,))
        if to_host:
            jac = jac.cpu().numpy()
            val = None if val is None else val.cpu().numpy()
        return (jac, val) if want_values else jac

    def render_warp_grad(self, matrix, size, wrt="source", **options):
        """The derivative of an affine view: ``sample_grad`` at the cell centres of ``blocks.warp_points(matrix, size)``,
        ``[*size, d, C]``.  ``wrt="source"``: per source pixel, as ``sample_grad`` gives it; ``wrt="view"``: per output cell,
        the chain rule through ``x = M (i + 0.5) + t`` applied on the device, ``J_view[..., m, c] = sum_l J[..., l, c] M[l, m]``.
        ``options`` are ``sample_grad``'s."""
        if wrt not in ("source", "view"):
            raise ValueError('render_warp_grad: wrt must be "source" or "view"')
        to_host = options.pop("to_host", True)
        want_values = options.get("want_values", False)
        res = self.sample_grad(blk.warp_points(matrix, size), to_host=False, **options)
        jac, val = res if want_values else (res, None)
        if wrt == "view":
            jac = _warp_chain(jac, matrix, self.dim_domain)
        if to_host:
            jac = jac.cpu().numpy()
            val = None if val is None else val.cpu().numpy()
        return (jac, val) if want_values else jac

    # hooks of _render
    def _engine_render_blend(self, params, active, axes, grid, extent, out, tdt, want_argmax, blend):
        # the engine reads the neighbours of this rank's blocks: with several ranks, everyone's parameters and list words
        # (small: a few hundred bytes per block) are gathered first; the images are summed as for blend = 0
        center = None
        if self.world_size > 1:
            dev = self._engine.device
            full = lambda t: torch.from_numpy(np.ascontiguousarray(sdist.allgather_blocks(t.cpu().numpy(), self.num_blocks))).to(dev)
            params = {k: full(v) for k, v in params.items()}
            active = None if active is None else full(active)
            if self._mus_grid is not None and int(self.quantization_mode) >= 2:
                center = torch.from_numpy(np.ascontiguousarray(sdist.allgather_blocks(self._mus_grid, self.num_blocks),
                                                               dtype=np.float32)).to(dev)
        return self._engine.render_blend(params, active, axes, grid, extent, blend, first_block=self.lo,
                                         num_blocks=self.hi - self.lo, out=out, dtype=tdt, want_argmax=want_argmax,
                                         center_grid=center)

    def _local_rparams(self):
        rp = {k: np.ascontiguousarray(self.rparams[k][self.lo:self.hi], dtype=np.float32) for k in PARAM_NAMES}
        return _pad_kernels(rp, self._kp)

    def _render_lists(self, quantized):
        # the kernel lists of the pass behind get_reconstruction() while that reconstruction is current (the pass prunes
        # its lists only after it has evaluated with them), the current lists otherwise
        if self.valid and not quantized and getattr(self, "_recon_active", None) is not None:
            return self._recon_active
        return self._active

    def _render_grid(self, m):
        n = self.batch_size_valued
        extent = [max(1, int(self.image.shape[l]) * m[l] // n[l]) for l in range(self.dim_domain)]   # crops ragged padding
        return self.grid, extent, [blk.render_axis(n[l], m[l]) for l in range(self.dim_domain)]

    def _engine_render(self, params, active, axes, m, grid, extent, out, tdt, want_argmax):
        return self._engine.render(params, active, axes, grid, extent, first_block=self.lo, out=out, dtype=tdt,
                                   want_argmax=want_argmax)

    def _global_ids(self, am, bid, own):
        # global kernel id = block index * K + kernel (as _assemble_one forms it); -1: none, or another rank's block
        return torch.where(own & (am != 255), am + bid * self.kernels, torch.full_like(am, -1))

    def get_weight_matrix(self):
        if not self.valid:
            self.run_batched(train=False, update_reconstruction=True)
        return self.weight_matrix

    # -- checkpoint / restore (replaces the tf.train.Saver of smoe.py:1066-1077) ---------------
    def checkpoint(self, path):
        st = {"params": {k: v.cpu().numpy().copy() for k, v in self._params.items()},
              "best": {k: v.cpu().numpy().copy() for k, v in self._best.items()},
              "m": {k: v.cpu().numpy().copy() for k, v in self._state.m.items()},
              "v": {k: v.cpu().numpy().copy() for k, v in self._state.v.items()},
              "beta_pow": (float(self._state.c.beta1_power), float(self._state.c.beta2_power)),
              "step": int(self._state.c.step), "active": self._active.cpu().numpy(),
              "diverged": self._diverged.cpu().numpy(), "iter": self.iter, "losses": self.losses,
              "mses": self.mses, "num_pis": self.num_pis, "shard": (self.lo, self.hi, self.num_blocks),
              # what train() needs to continue exactly where it stopped: the per-block best losses behind the best
              # snapshot, the iteration-0 losses of the per-block stop rule (smoe.py:1565-1570) and the best scalars
              "best_loss_blocks": None if self._best_loss_blocks is None else self._best_loss_blocks.cpu().numpy(),
              "loss0": None if self._loss0 is None else self._loss0.cpu().numpy(),
              "best_loss": self.best_loss, "best_mse": self.best_mse}
        with open(path if self.world_size == 1 else f"{path}.rank{self.rank}", "wb") as fd:
            pickle.dump(st, fd)
        return path

    def restore(self, path):
        with open(path if self.world_size == 1 else f"{path}.rank{self.rank}", "rb") as fd:
            st = pickle.load(fd)
        assert tuple(st["shard"]) == (self.lo, self.hi, self.num_blocks), "checkpoint belongs to another sharding"
        dev = self._engine.device
        for k in PARAM_NAMES:
            self._params[k].copy_(torch.from_numpy(st["params"][k]).to(dev))
            self._best[k].copy_(torch.from_numpy(st["best"][k]).to(dev))
            self._state.m[k].copy_(torch.from_numpy(st["m"][k]).to(dev))
            self._state.v[k].copy_(torch.from_numpy(st["v"][k]).to(dev))
        self._state.c.beta1_power, self._state.c.beta2_power = st["beta_pow"]
        self._state.c.step = st["step"]
        self._active.copy_(torch.from_numpy(st["active"]).to(dev))
        self._diverged.copy_(torch.from_numpy(st["diverged"]).to(dev))
        self.iter = st["iter"]
        self.losses, self.mses, self.num_pis = st["losses"], st["mses"], st["num_pis"]
        self._best_loss_blocks = None if st.get("best_loss_blocks") is None else torch.from_numpy(st["best_loss_blocks"]).to(dev)
        self._loss0 = None if st.get("loss0") is None else torch.from_numpy(st["loss0"]).to(dev)
        self.best_loss, self.best_mse = st.get("best_loss"), st.get("best_mse", [])
        self.valid = False


# =====================================================================================================
# shared-kernel image mode: the reference's whole-image fit
# =====================================================================================================
def _default_shared_factory(cfg, device):
    from .engine import SharedEngine
    return SharedEngine(cfg, device)


class SharedSmoe(_SmoeBase):
    """``Smoe`` with ONE global kernel set, as the reference fits whole images
    (``Smoe(image, kernels_per_dim=[12, 12], batch_size=[32, 32])``): ``kernels_per_dim`` is the
    global kernel grid, ``batch_size`` the pixel batch of a pass (smoe.py:231-247), every batch keeps
    its own kernel list (smoe.py:315,1763-1766,2287-2365), the gradients of all batches are
    accumulated and one Adam step follows (smoe.py:1148-1150,1788).  ``get_params()`` returns the
    reference's layout exactly (leading axis = kernels).  Multi-GPU: the BATCHES are sharded over
    ranks and the accumulated gradient buffer is all-reduced (RCCL) before the Adam step.
    ``overlap_of_batches`` > 0: the halo of every batch takes part in the kernel-list influence test
    only (its loss is cropped, smoe.py:909-923)."""
    _unit = "batch"

    def __init__(self, image, kernels_per_dim=None, train_pis=True, init_params=None, start_batches=1,
                 batch_size=None, train_gammas=True, train_musx=True, use_determinant=False, normalize_pis=True,
                 use_yuv=True, precision=8, iter_offset=0, margin=0.5, overlap_of_batches=0, device=None,
                 engine_factory=None, quantization_mode=0, quantize_pis=False, bit_depths=None, lower_bounds=None,
                 upper_bounds=None, only_y_gamma=False, use_diff_center=False, ssim_opt=False, train_inverse_cov=True,
                 radial_as=False, loss_mask=None, kernel_count_as_norm_l1=False, **unsupported):
        for name, val in unsupported.items():
            if val:
                raise NotImplementedError(f"SharedSmoe({name}=...) is outside the hot path (SURVEY section 8)")
        self._set_quantizer(quantization_mode, quantize_pis, bit_depths, lower_bounds, upper_bounds)
        self.kernel_count_as_norm_l1 = bool(kernel_count_as_norm_l1)                  # smoe.py:1022-1027
        assert kernels_per_dim is not None or init_params is not None, \
            "You need to specify the kernel grid size or give initial parameters."
        image = self._set_image(image, precision, margin, use_yuv, only_y_gamma)
        d = self.dim_domain
        self.use_determinant = use_determinant
        self.train_pis, self.train_gammas, self.train_musx = train_pis, train_gammas, train_musx
        self.radial_as = bool(radial_as)                                   # smoe.py:429-434,714-719
        self.train_inverse_cov = bool(train_inverse_cov)                  # smoe.py:41: the constructor default is True
        self.ssim_opt = bool(ssim_opt)                                    # smoe.py:929,980-1011: 1 - SSIM per batch
        self.use_diff_center = bool(use_diff_center)
        self.overlap = int(overlap_of_batches)                            # smoe.py:244
        bs = self._batch_shape(batch_size, start_batches)
        for ii in range(d):                                               # smoe.py:239-241
            if image.shape[ii] % bs[ii] > 0:
                raise ValueError("Required BatchSize is not compatible to input dimensions")
        self.batch_size_valued = bs
        self.batch_size = tuple(int(b) + 2 * self.overlap for b in bs)    # smoe.py:245
        self.Nb = int(np.prod(bs))
        blocks_all, _ = blk.image_to_blocks(image, bs)
        self.num_batches = self.start_batches = blocks_all.shape[0]
        self.rank, self.world_size = sdist.world()
        self.lo, self.hi = sdist.shard_range(self.num_batches, self.rank, self.world_size)
        if init_params:
            p0 = {k: np.ascontiguousarray(init_params[k], dtype=np.float32) for k in PARAM_NAMES}
            self.musX_init = p0["musX"]
        else:
            kpd = list(kernels_per_dim)
            if len(kpd) == 1:
                kpd = kpd * d
            p0 = {k: v[0] for k, v in blk.init_block_params(image[None], kpd, normalize_pis, self.train_inverse_cov).items()}
            self.musX_init = blk.gen_domain_grid(kpd, d)
        if self.radial_as:                    # one steering value per kernel: A_init[:, 0, 0] tiled over the diagonal
            a0 = p0["A_diagonal"] if p0["A_diagonal"].ndim == 1 else p0["A_diagonal"][:, 0, 0]
            p0["A_diagonal"] = np.ascontiguousarray(a0[:, None, None] * np.eye(d, dtype=np.float32))
        self.kernels = self._kp = self.start_pis = self.kernel_count = p0["pis"].shape[0]      # no padding kernels here
        # use_diff_center (smoe.py:390-394,746-747): the trained variable is the offset from the kernel grid; the
        # engine works on grid + offset, the getters subtract the grid
        self._mus_grid = np.ascontiguousarray(p0["musX"]).copy() if self.use_diff_center else None
        dev = self._start_engine(engine_factory or _default_shared_factory, device)
        self._target = torch.from_numpy(blk.to_planar(blocks_all[self.lo:self.hi])).to(dev)
        self._params = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p0.items()}
        self._best = {k: v.clone() for k, v in self._params.items()}
        self._state = self._engine.new_adam_state(self._params)
        self._lists = self._engine.new_lists(self.hi - self.lo)           # smoe.py:315
        # loss_mask (smoe.py:1674-1677): per-pixel loss weights, cut into the batches like the image
        self.loss_mask = loss_mask
        self._loss_w = None
        if loss_mask is not None:
            if self.ssim_opt:
                raise NotImplementedError("ssim_opt ignores loss weights (as the reference does)")
            lm, _ = blk.image_to_blocks(np.asarray(loss_mask, dtype=np.float32)[..., None], bs)
            self._loss_w = torch.from_numpy(np.ascontiguousarray(lm.reshape(self.num_batches, -1))).to(dev)
            self._engine.set_loss_weights(self._loss_w)
        self._reset_histories(iter_offset)
        self._recon_lists = self._qrecon_lists = None
        self.reconstruction_image = self.weight_matrix_argmax = self.qreconstruction_image = None
        self.qparams = self.rparams = None                                # quantizer.py products (leading axis 1 = the model)

    def _config(self, **common):
        return SharedConfig(image_shape=tuple(self.image.shape[:self.dim_domain]), batch_shape=self.batch_size_valued,
                            overlap=self.overlap, **common)

    def _engine_created(self):
        self._hand_over_center_grid()
        if getattr(self, "_loss_w", None) is not None:                    # a re-created engine needs the weights again
            self._engine.set_loss_weights(self._loss_w)

    @property
    def kernel_list_per_batch(self):
        bits = self._lists.cpu().numpy().view(np.uint32)
        K = self.kernels
        return [np.array([(row[k >> 5] >> (k & 31)) & 1 for k in range(K)], dtype=bool) for row in bits]

    def _global(self, loss, sse):
        s = torch.stack([loss.double().sum(), sse.double().sum()])
        sdist.allreduce_sum_(s)
        s = s.cpu().numpy()
        loss_val = float(s[0]) * self.Nb / self.num_pixel                              # smoe.py:1758
        mse_val = float(s[1]) / (self.num_pixel * self.channels) * (2 ** self.precision) ** 2
        return loss_val, mse_val, int(self._count_pis().item())      # not reduced: the parameters are replicated

    def _quantize(self):
        """quantize_params + rescaler (quantizer.py:4-145) on the global kernel set (one model = leading axis 1)."""
        from .quantizer import quantize_params, rescaler
        self.qparams = quantize_params(self, {k: v[None] for k, v in self.get_params().items()})
        if self.quantization_mode == 1:
            self.rparams = rescaler(self, self.qparams)

    def run_batched(self, pis_l1=0, u_l1=0, sv_l1_sub_l2=0, train=True, update_reconstruction=False,
                    with_quantized_params=False, **kw):
        for name, val in kw.items():
            if val not in (False, None, 100):
                raise NotImplementedError(f"run_batched({name}=...) is outside the hot path")
        self._make_engine(pis_l1, u_l1)
        eng, nb = self._engine, self.hi - self.lo
        dev = eng.device
        if with_quantized_params:                                         # smoe.py:1688-1689: the lists are not touched
            rp = self._quantized_params()
            self.qvalid = False
            out = eng.forward(self._target, rp, self._lists, first_batch=self.lo, want_recon=update_reconstruction,
                              want_argmax=False, update_lists=False)
            if update_reconstruction:
                self._qrecon_lists = self._lists.clone()    # what this pass evaluated with (render(quantized=True))
                bs, d = self.batch_size_valued, self.dim_domain
                rec = sdist.allgather_blocks(blk.from_planar(out["recon"].cpu().numpy(), bs), self.num_batches)
                self.qreconstruction_image = blk.blocks_to_image(rec, self.image.shape[:d], bs)
                self.qvalid = True
            loss_val, mse_val, num_pi = self._global(out["loss"], out["sse"])
            return loss_val, mse_val, num_pi, 0
        self.valid = False
        if train:
            assert self.optimizer1 is not None, "no optimizer found, you have to specify one!"
            loss = torch.zeros((nb,), dtype=torch.float32, device=dev)
            sse = torch.zeros((nb,), dtype=torch.float32, device=dev)
            eng.accumulate(self._target, self._params, self._lists, first_batch=self.lo, loss_out=loss, sse_out=sse)
            if self.world_size > 1:
                sdist.allreduce_sum_(eng.grad_buffer())                    # the gradient exchange of the pass
            eng.apply(self._params, self._state)
        else:
            if update_reconstruction:
                self._recon_lists = self._lists.clone()     # what this pass evaluates with, before it prunes (render)
            out = eng.forward(self._target, self._params, self._lists, first_batch=self.lo,
                              want_recon=update_reconstruction, want_argmax=update_reconstruction)
            loss, sse = out["loss"], out["sse"]
            if update_reconstruction:
                bs, d = self.batch_size_valued, self.dim_domain
                rec = sdist.allgather_blocks(blk.from_planar(out["recon"].cpu().numpy(), bs), self.num_batches)
                self.reconstruction_image = blk.blocks_to_image(rec, self.image.shape[:d], bs)
                am = out["argmax"].cpu().numpy().astype(np.int64).reshape((nb,) + bs)
                am = sdist.allgather_blocks(am, self.num_batches)
                self.weight_matrix_argmax = blk.blocks_to_image(am[..., None], self.image.shape[:d], bs)[..., 0]
                self.valid = True
        loss_val, mse_val, num_pi = self._global(loss, sse)
        return loss_val, mse_val, num_pi, 0

    def train(self, num_iter, val_iter=100, ukl_iter=None, optimizer1=None, optimizer2=None, optimizer3=None,
              grad_clip_value_abs=None, pis_l1=0, u_l1=0, callbacks=(), **kw):
        ukl_iter = self._begin_train(val_iter, ukl_iter, optimizer1, optimizer2, optimizer3, grad_clip_value_abs)
        self._make_engine(pis_l1, u_l1)
        _train_loop(self, num_iter, val_iter, ukl_iter, pis_l1, u_l1, callbacks)

    # hooks of _train_loop
    def _after_first_evaluation(self):
        pass

    def _fit_iterations(self, n):
        eng = self._engine
        if self.world_size == 1:                                             # n x (accumulate; apply) in one call
            eng.fit(self._target, self._params, self._state, self._lists, n)
        else:
            for _ in range(n):
                eng.accumulate(self._target, self._params, self._lists, first_batch=self.lo)
                sdist.allreduce_sum_(eng.grad_buffer())                      # the gradient exchange of the pass
                eng.apply(self._params, self._state)

    def _readmit_kernels(self):
        self._engine.update_kernel_list(self._params, self._lists, first_batch=self.lo)

    def _keep_best(self, loss_val):
        if not self.best_loss or loss_val < self.best_loss:                  # smoe.py:1574-1576
            self.best_loss = loss_val
            for k in PARAM_NAMES:
                self._best[k].copy_(self._params[k])

    def _host_params(self, p):
        out = {k: v.cpu().numpy().copy() for k, v in p.items()}
        if self._mus_grid is not None:                     # use_diff_center: report the trained offsets
            out["musX"] = out["musX"] - self._mus_grid
        if self.radial_as:                                 # the reference's (K,) variable
            out["A_diagonal"] = np.ascontiguousarray(out["A_diagonal"][:, 0, 0])
        return out

    def get_params(self):
        return self._host_params(self._params)

    def get_best_params(self):
        return self._host_params(self._best)

    def render(self, scale=None, samples_per_block=None, dtype=np.float32, quantized=False, want_argmax=False,
               to_host=True, use_lists=True, blend=0.0):
        """Decode the fitted whole-image model on another sampling grid, on the device (the engine's ``render``).  The
        model is ONE continuous function over the image domain -- no block seams -- so zooming, a finer pitch or frames
        between the fitted ones are "evaluate the same model somewhere else"; no pixel is interpolated.
        ``scale``: a number or one per axis, ``m_l = round(scale_l * n_l)`` samples per batch (at least 1, ``n`` =
        ``batch_size_valued``); ``samples_per_block``: the ``m_l`` themselves (a number or one per axis); neither: the
        training lattice.  Output extent ``E_l = grid_l * m_l`` (the image is a multiple of the batch: nothing to crop),
        layout ``[*E, C]`` as ``get_reconstruction()``; ``dtype`` float32 (lattice values) or uint8 (lattice indices).
        Sample positions: ``blocks.render_axis(image.shape[l], E_l)`` on the IMAGE axis -- ``E_l == image.shape[l]`` is the
        training lattice itself, otherwise cell centres over the image's pixel footprint; sample ``j`` lies in the
        footprint of batch ``j // m_l`` and is evaluated with that batch's kernel list.
        ``quantized``: render ``rparams`` (what ``get_qreconstruction`` evaluates).  ``want_argmax``: also the map of
        global kernel ids ``[*E]`` (int64; -1 where no kernel has influence on the sample).  ``to_host=False`` returns
        device tensors.
        Lists: the ones the pass behind ``get_reconstruction()`` (``quantized``: ``get_qreconstruction()``) evaluated with
        while that reconstruction is current (a pass prunes the lists only after it has evaluated with them), the current
        ones otherwise.  A kernel that was pruned
        from a batch because it had no influence on the batch's PIXELS may be missing at an in-between sample near the
        batch's edge.  ``use_lists=False`` passes no lists: every kernel with a positive prior, everywhere -- slower, and
        free of the list boundaries.  (It is not the same function even on the training lattice: a pruned kernel's masked
        weight was zero, but its gate still sat in the normaliser of the pass that pruned it.)
        Several ranks: every rank renders its batches and the images are summed; the result is the same on every rank
        and for every number of ranks.
        ``blend``: accepted for symmetry with ``Smoe.render`` and must be 0 -- a whole-image model has no block seams."""
        if np.any(np.asarray(blend, dtype=np.float64) != 0):
            raise ValueError("render: blend is for block models; a whole-image model has no block seams")
        return self._render(scale, samples_per_block, dtype, quantized, want_argmax, to_host, use_lists)

    # -- decoding at arbitrary points and in viewports ------------------------------------------
    # (``Smoe`` calls these sample / render_view / render_warp; here they carry names of their own.)
    def _eval_model(self, who, dtype, quantized, use_lists, method):
        """What the point and viewport decoders take: the torch dtype, the engine, the parameters and the kernel lists of
        ALL batches on this rank's device (``render``'s lists; with several ranks everyone's are gathered -- the parameters
        are replicated anyway)."""
        npdt = np.dtype(dtype)
        if npdt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError(f"{who}: dtype must be float32 or uint8")
        tdt = torch.uint8 if npdt == np.dtype(np.uint8) else torch.float32
        eng = self._engine
        if not hasattr(eng, method):
            raise NotImplementedError(f"this engine has no {method}()")
        params = self._quantized_params() if quantized else self._params
        lists = self._render_lists(quantized) if use_lists else None
        if lists is not None and self.world_size > 1:
            full = sdist.allgather_blocks(lists.cpu().numpy(), self.num_batches)
            lists = torch.from_numpy(np.ascontiguousarray(full)).to(eng.device)
        return tdt, eng, params, lists

    @staticmethod
    def _eval_result(res, want_argmax, to_host):
        img, ids = res if want_argmax else (res, None)
        ids = None if ids is None else ids.to(torch.int64)
        if to_host:
            img = img.cpu().numpy()
            ids = None if ids is None else ids.cpu().numpy()
        return (img, ids) if want_argmax else img

    def _eval_points_arg(self, who, points, dev):
        """``points`` ``[..., d]`` (array-like or a tensor) as the engine takes them -- a contiguous float32 ``[N, d]`` tensor on
        ``dev`` -- and their leading shape."""
        d = self.dim_domain
        pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points), dtype=np.float32))
        if pts.dim() < 1 or pts.shape[-1] != d:
            raise ValueError(f"{who}: points need a trailing axis of {d} coordinates")
        return pts.to(device=dev, dtype=torch.float32).reshape(-1, d).contiguous(), tuple(pts.shape[:-1])

    def eval_points(self, points, dtype=np.float32, quantized=False, want_argmax=False, to_host=True, use_lists=True):
        """The model's value at arbitrary positions, on the device (the engine's ``sample``; include/smoe_hip.h:
        smoe_shared_sample) -- ``Smoe.sample`` for a whole-image model: a rotated or warped view, a profile along a line, a
        few thousand probes; no pixel is interpolated.  ``points``: array-like or a device tensor ``[..., d]`` of float32
        positions in source pixels, in the image's axis order (pixel ``q`` covers ``[q, q + 1)``).  A point is evaluated with
        the kernel list of the batch it lies in (``blocks.point_blocks(points, batch_size_valued, grid, image.shape)[1]``)
        at the image-unit coordinate ``(x - 0.5) / (S - 1)`` (``blocks.point_blocks(points, image.shape, [1] * d,
        image.shape)[2]``).  Returns ``[..., C]``; a position outside the image (NaN, ``< 0`` or ``>= image.shape[l]`` on any
        axis) gives 0.  ``dtype``, ``quantized``, ``use_lists`` and the lists are ``render``'s; with ``want_argmax`` also the
        global kernel ids ``[...]`` (int64; -1: no kernel has influence, or outside).  The pixel centres ``q + 0.5`` give
        ``render()`` bit for bit.  ``to_host=False`` returns device tensors.  Several ranks: the lists are gathered and every
        rank evaluates all points; the result is the same on every rank and for every number of ranks.
        Neighbouring points are cheap, scattered ones are not: the device walks the distinct batches among 1024 consecutive
        points one after the other."""
        tdt, eng, params, lists = self._eval_model("eval_points", dtype, quantized, use_lists, "sample")
        pts, lead = self._eval_points_arg("eval_points", points, eng.device)
        res = eng.sample(params, lists, pts, dtype=tdt, want_argmax=want_argmax)
        img, ids = res if want_argmax else (res, None)
        img = img.reshape(lead + (self.channels,))
        ids = None if ids is None else ids.reshape(lead)
        return self._eval_result((img, ids) if want_argmax else img, want_argmax, to_host)

    def _view_window(self, who, window, size, scale):
        """``eval_view``'s window / size / scale, checked: one ``(lo, hi)`` per axis and the extent ``E``."""
        d = self.dim_domain
        shape = [int(v) for v in self.image.shape[:d]]
        window = [None] * d if window is None else list(window)
        if len(window) != d:
            raise ValueError(f"{who}: window needs one (lo, hi) per axis ({d})")
        win = [(0.0, float(shape[l])) if w is None else (float(w[0]), float(w[1])) for l, w in enumerate(window)]
        for l, (lo, hi) in enumerate(win):
            if not (0.0 <= lo < hi <= float(shape[l])):
                raise ValueError(f"{who}: window[{l}] must satisfy 0 <= lo < hi <= {shape[l]}")
        if size is not None and scale is not None:
            raise ValueError(f"{who}: give size or scale, not both")
        if size is not None:
            E = [int(v) for v in np.atleast_1d(size)]
            E = E * d if len(E) == 1 else E
            if len(E) != d or min(E) < 1:
                raise ValueError(f"{who}: size needs {d} entries >= 1")
        else:
            sc = list(np.atleast_1d(1 if scale is None else scale))
            sc = sc * d if len(sc) == 1 else sc
            if len(sc) != d:
                raise ValueError(f"{who}: scale needs one value or {d}")
            E = [max(1, int(round((hi - lo) * float(v)))) for (lo, hi), v in zip(win, sc)]
        return win, E

    def _view_tables(self, win, E):
        """A checked window and extent (``_view_window``) as the engine's tables (numpy): per axis the coordinates and the
        batch indices of the ``E_l`` samples (``blocks.view_axis``)."""
        d, n = self.dim_domain, self.batch_size_valued
        shape = [int(v) for v in self.image.shape[:d]]
        axes, batches = [], []
        for l in range(d):
            axes.append(blk.view_axis(shape[l], 1, shape[l], win[l][0], win[l][1], E[l])[3])
            first, nblocks, start, _ = blk.view_axis(n[l], shape[l] // n[l], shape[l], win[l][0], win[l][1], E[l])
            batches.append((first + np.repeat(np.arange(nblocks), np.diff(start))).astype(np.int32))
        return axes, batches

    def eval_view(self, window, size=None, scale=None, dtype=np.float32, quantized=False, want_argmax=False,
                  to_host=True, use_lists=True, taps=None):
        """Decode a viewport: the axis-aligned ``window`` of the image domain at the output ``size``, on the device (the
        engine's ``render_view``; include/smoe_hip.h: smoe_shared_render_view) -- ``Smoe.render_view`` for a whole-image
        model.  Only the window is computed and stored: an 8x detail, a fit-to-window zoom, a thumbnail with fewer samples
        than batches, one frame of a video.  ``window``: one ``(lo, hi)`` per axis in source pixels (pixel ``q`` covers
        ``[q, q + 1)``, ``0 <= lo < hi <= image.shape[l]``; None for an axis, or for all: the whole axis).  ``size``: the
        ``E_l`` output samples per axis, or ``scale`` (a number or one per axis): ``E_l = max(1, round((hi - lo) *
        scale_l))``; not both, neither: scale 1.  Sample ``i`` sits at ``lo + (i + 0.5)(hi - lo) / E_l``: its coordinate is
        ``blocks.view_axis(S, 1, S, lo, hi, E)[3]`` on the image axis of ``S`` pixels, its batch the one of
        ``blocks.view_axis(n, grid_l, S, lo, hi, E)`` -- a window that is a crop of a ``render`` grid gives exactly that
        crop.  The other options and the return value are ``eval_points``'s, ``[*E, C]``.
        ``taps``: None (the default) or all ones: one position per sample, as above.  Otherwise (a number, one per axis or
        ``"auto"``) every sample is the mean over ``taps[l]`` taps per axis inside its cell -- ``eval_points_area`` at the
        mesh of ``blocks.view_positions(lo, hi, E)`` with the footprint ``diag((hi - lo) / E)``: a thumbnail that does not
        alias.  ``want_argmax`` is refused then (an average has no single kernel)."""
        win, E = self._view_window("eval_view", window, size, scale)
        foot = np.diag([(hi - lo) / e for (lo, hi), e in zip(win, E)])
        tp = self._taps_arg("eval_view", taps, foot)
        if tp is not None:
            if want_argmax:
                raise ValueError("eval_view: want_argmax needs taps=None (an average has no single kernel)")
            axes = [blk.view_positions(lo, hi, e) for (lo, hi), e in zip(win, E)]     # view_axis' x_i, rounded once
            pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
            return self.eval_points_area(pts, foot, taps=tp, dtype=dtype, quantized=quantized, to_host=to_host,
                                         use_lists=use_lists)
        axes, batches = self._view_tables(win, E)
        tdt, eng, params, lists = self._eval_model("eval_view", dtype, quantized, use_lists, "render_view")
        axes, batches = ([torch.from_numpy(t).to(eng.device) for t in tabs] for tabs in (axes, batches))
        res = eng.render_view(params, lists, axes, batches, dtype=tdt, want_argmax=want_argmax)
        return self._eval_result(res, want_argmax, to_host)

    def eval_warp(self, matrix, size, taps=None, **options):
        """An affine view of the model: ``eval_points(blocks.warp_points(matrix, size), **options)`` -- ``Smoe.render_warp``
        for a whole-image model.  ``matrix = [M | t]`` ``[d, d + 1]`` maps the cell centre ``i + 0.5`` of output index ``i``
        to the source position ``M (i + 0.5) + t`` in source pixels.  Returns the image ``[*size, C]`` (0 where the view
        leaves the image).  ``taps``: None (the default) or all ones: that call.  Otherwise (a number, one per view axis or
        ``"auto"``) ``eval_points_area`` at the same positions with the footprint ``M`` -- a zoomed-out warp that does not
        alias; ``options`` are ``eval_points_area``'s then, and ``want_argmax`` is a ``ValueError``."""
        pts = blk.warp_points(matrix, size)
        M = np.asarray(matrix, dtype=np.float64)[:, :self.dim_domain]
        tp = self._taps_arg("eval_warp", taps, M)
        if tp is None:
            return self.eval_points(pts, **options)
        if options.pop("want_argmax", False):
            raise ValueError("eval_warp: want_argmax needs taps=None (an average has no single kernel)")
        return self.eval_points_area(pts, M, taps=tp, **options)

    def eval_points_area(self, points, footprint, taps="auto", dtype=np.float32, quantized=False, want_mean=False,
                         want_count=False, to_host=True, use_lists=True):
        """Anti-aliased ``eval_points``, on the device (the engine's ``sample_area``; include/smoe_hip.h:
        smoe_shared_sample_area) -- ``Smoe.sample_area`` for a whole-image model: every point is the centre of an output cell,
        and its result is the mean of the model over a regular grid of taps inside the cell, put on the lattice.  Every tap
        is evaluated with the kernel list of the batch IT lies in, so a cell that straddles batches is the mean of what
        ``eval_points`` gives at its taps.  ``footprint`` ``[d, d]`` in source pixels: column ``m`` is the edge vector of a
        cell along view axis ``m`` (``M`` of an affine view, ``diag((hi - lo) / E)`` of a viewport); one footprint serves all
        points.  ``taps``: a number, one per view axis (1 .. 16, product at most 64) or ``"auto"``
        (``blocks.footprint_taps``).  Positions: ``blocks.area_taps``.  Taps outside the image are left out of the mean; a
        cell with no tap inside gives 0.  ``points``, ``dtype``, ``quantized``, ``use_lists`` and the lists are
        ``eval_points``'s.  Returns ``[..., C]``; with ``want_mean`` also the float32 means before the lattice ``[..., C]``,
        with ``want_count`` the uint8 number of taps inside ``[...]``.  ``to_host=False`` returns device tensors.  Several
        ranks: as ``eval_points``."""
        tdt, eng, params, lists = self._eval_model("eval_points_area", dtype, quantized, use_lists, "sample_area")
        tp = self._taps_arg("eval_points_area", taps, footprint) or [1] * self.dim_domain
        pts, lead = self._eval_points_arg("eval_points_area", points, eng.device)
        res = eng.sample_area(params, lists, pts, footprint, tp, dtype=tdt, want_mean=want_mean, want_count=want_count)
        res = list(res) if isinstance(res, tuple) else [res]
        res[0] = res[0].reshape(lead + (self.channels,))
        if want_mean:
            res[1] = res[1].reshape(lead + (self.channels,))
        if want_count:
            res[-1] = res[-1].reshape(lead)
        if to_host:
            res = [t.cpu().numpy() for t in res]
        return tuple(res) if len(res) > 1 else res[0]

    def eval_points_area_each(self, points, footprints, taps="auto", dtype=np.float32, quantized=False, want_mean=False,
                              want_count=False, to_host=True, use_lists=True):
        """``eval_points_area`` with a footprint of its own for every point, on the device (the engine's ``sample_area_each``;
        include/smoe_hip.h: smoe_shared_sample_area_each) -- ``Smoe.sample_area_each`` for a whole-image model: a view whose
        magnification varies across the output, a perspective view, a lens or stabilisation map, any dense lookup map.
        ``points`` ``[..., d]`` and ``footprints`` ``[..., d, d]`` (arrays or device tensors; column ``m`` of a footprint is the
        edge vector of that sample's cell along view axis ``m``, source pixels).  ``taps``: ``"auto"``
        (``blocks.footprint_taps_each``: one tap per source pixel covered, per point), a number or one per view axis
        (broadcast), or an integer array ``[..., d]``.  Positions: ``blocks.area_taps_each``.  A point is the result of
        ``eval_points_area`` with its footprint and taps, bit for bit.  A point whose taps are outside 1 .. 16, multiply to
        more than 64 or whose footprint is not finite is void: 0, mean 0, count 0.  Everything else, and what is returned, is
        ``eval_points_area``'s."""
        d = self.dim_domain
        who = "eval_points_area_each"
        tdt, eng, params, lists = self._eval_model(who, dtype, quantized, use_lists, "sample_area_each")
        pts, lead = self._eval_points_arg(who, points, eng.device)
        if torch.is_tensor(footprints):
            foot = footprints
        else:
            fa = np.asarray(footprints)
            if fa.dtype.kind not in "fiu":
                raise ValueError(f"{who}: footprints must be numbers")
            foot = torch.from_numpy(np.ascontiguousarray(fa, dtype=np.float32))
        if tuple(foot.shape) != lead + (d, d) or not foot.dtype.is_floating_point:
            raise ValueError(f"{who}: footprints must be floating point {lead + (d, d)}")
        foot = foot.to(device=eng.device, dtype=torch.float32).reshape(-1, d, d).contiguous()
        tp = self._taps_each_arg(who, taps, foot, lead)
        res = eng.sample_area_each(params, lists, pts, foot, tp, dtype=tdt, want_mean=want_mean, want_count=want_count)
        res = list(res) if isinstance(res, tuple) else [res]
        res[0] = res[0].reshape(lead + (self.channels,))
        if want_mean:
            res[1] = res[1].reshape(lead + (self.channels,))
        if want_count:
            res[-1] = res[-1].reshape(lead)
        if to_host:
            res = [t.cpu().numpy() for t in res]
        return tuple(res) if len(res) > 1 else res[0]

    def eval_projective(self, H, size, taps="auto", **options):
        """A projective view of the model, anti-aliased: ``eval_points_area_each`` at ``blocks.projective_points(H, size)`` --
        ``Smoe.render_projective`` for a whole-image model.  ``H`` ``[d + 1, d + 1]`` maps the cell centre ``c = i + 0.5`` of
        output index ``i`` to ``(H[:d, :d] c + H[:d, d]) / (H[d, :d] . c + H[d, d])`` in source pixels; every sample is
        averaged over its own footprint, the analytic Jacobian of the map there.  Returns the image ``[*size, C]``; samples
        behind the horizon and where the view leaves the image give 0.  ``taps``: ``"auto"`` (the default), a number or one
        per view axis; None or all ones: ``eval_points(points)``.  ``options`` are ``eval_points_area_each``'s
        (``eval_points``'s with ``taps`` None)."""
        try:
            pts, foot, _ = blk.projective_points(H, size)
        except ValueError as e:
            raise ValueError(f"eval_projective: {e}") from None
        if self._ones_taps("eval_projective", taps):
            return self.eval_points(pts, **options)
        return self.eval_points_area_each(pts, foot, taps=taps, **options)

    def eval_map(self, points, taps="auto", **options):
        """A dense lookup map of the model, anti-aliased -- ``Smoe.render_map`` for a whole-image model: ``points``
        ``[*size, d]`` (an array or a device tensor) holds the source position of every output sample, and every sample is
        averaged over its own footprint ``blocks.map_footprints(points)`` (central differences of the map; made on the device
        for a device tensor).  Returns ``[*size, C]``.  ``taps`` and ``options`` as in ``eval_projective``."""
        d = self.dim_domain
        if (points.dim() if torch.is_tensor(points) else np.ndim(points)) != d + 1 or tuple(points.shape)[-1] != d:
            raise ValueError(f"eval_map: points must be [*size, {d}] with {d} view axes")
        if self._ones_taps("eval_map", taps):
            return self.eval_points(points, **options)
        if torch.is_tensor(points):
            if not points.dtype.is_floating_point:
                raise ValueError("eval_map: points must be floating point")
            p32 = points.to(torch.float32)
            foot = map_footprints_torch(p32) if p32.is_cuda else torch.from_numpy(blk.map_footprints(p32.numpy()))
            return self.eval_points_area_each(p32, foot, taps=taps, **options)
        pa = np.asarray(points)
        if pa.dtype.kind not in "fiu":
            raise ValueError("eval_map: points must be numbers")
        pa = pa.astype(np.float32)
        return self.eval_points_area_each(pa, blk.map_footprints(pa), taps=taps, **options)

    # -- the exact spatial derivative at the same points ----------------------------------------
    @staticmethod
    def _grad_result(jac, val, want_values, to_host):
        if to_host:
            jac = jac.cpu().numpy()
            val = None if val is None else val.cpu().numpy()
        return (jac, val) if want_values else jac

    def eval_points_grad(self, points, quantized=False, want_values=False, to_host=True, use_lists=True):
        """The model's exact spatial derivative at arbitrary positions, on the device (the engine's ``sample_grad``;
        include/smoe_hip.h: smoe_shared_sample_grad) -- ``Smoe.sample_grad`` for a whole-image model, which is one continuous
        function without block seams: an edge map, a structure tensor, the temporal slope of a video model, an alignment
        step.  Differences of ``eval_points`` sit on the 8-bit lattice; this is the closed-form derivative of the value before
        the lattice, with the gate mask and the clip held piecewise constant.  ``points``, ``quantized``, ``use_lists`` and
        the lists are ``eval_points``'s.  Returns ``[..., d, C]`` float32, ``jac[..., l, c] = dv_c / dx_l`` per source pixel
        (0 outside the image); with ``want_values`` also the float32 values before the lattice ``[..., C]``.
        ``to_host=False`` returns device tensors.  Several ranks: as ``eval_points``."""
        _, eng, params, lists = self._eval_model("eval_points_grad", np.float32, quantized, use_lists, "sample_grad")
        pts, lead = self._eval_points_arg("eval_points_grad", points, eng.device)
        res = eng.sample_grad(params, lists, pts, want_values=want_values)
        jac, val = res if want_values else (res, None)
        jac = jac.reshape(lead + (self.dim_domain, self.channels))
        val = None if val is None else val.reshape(lead + (self.channels,))
        return self._grad_result(jac, val, want_values, to_host)

    def eval_view_grad(self, window, size=None, scale=None, quantized=False, want_values=False, to_host=True, use_lists=True):
        """The derivative on a viewport: ``eval_view``'s ``window`` / ``size`` / ``scale`` and sample positions (the engine's
        ``render_view_grad``; include/smoe_hip.h: smoe_shared_render_view_grad).  Returns ``[*E, d, C]`` per SOURCE pixel,
        with ``want_values`` also ``[*E, C]``; the other options are ``eval_points_grad``'s."""
        axes, batches = self._view_tables(*self._view_window("eval_view_grad", window, size, scale))
        _, eng, params, lists = self._eval_model("eval_view_grad", np.float32, quantized, use_lists, "render_view_grad")
        axes, batches = ([torch.from_numpy(t).to(eng.device) for t in tabs] for tabs in (axes, batches))
        res = eng.render_view_grad(params, lists, axes, batches, want_values=want_values)
        jac, val = res if want_values else (res, None)
        return self._grad_result(jac, val, want_values, to_host)

    def eval_warp_grad(self, matrix, size, wrt="source", **options):
        """The derivative of an affine view: ``eval_points_grad`` at the cell centres of ``blocks.warp_points(matrix, size)``,
        ``[*size, d, C]`` -- ``Smoe.render_warp_grad`` for a whole-image model.  ``wrt="source"``: per source pixel;
        ``wrt="view"``: per output cell, the chain rule through ``x = M (i + 0.5) + t`` applied on the device,
        ``J_view[..., m, c] = sum_l J[..., l, c] M[l, m]``.  ``options`` are ``eval_points_grad``'s."""
        if wrt not in ("source", "view"):
            raise ValueError('eval_warp_grad: wrt must be "source" or "view"')
        to_host = options.pop("to_host", True)
        want_values = options.get("want_values", False)
        res = self.eval_points_grad(blk.warp_points(matrix, size), to_host=False, **options)
        jac, val = res if want_values else (res, None)
        if wrt == "view":
            jac = _warp_chain(jac, matrix, self.dim_domain)
        return self._grad_result(jac, val, want_values, to_host)

    # hooks of _render
    def _local_rparams(self):
        return {k: np.ascontiguousarray(self.rparams[k][0], dtype=np.float32) for k in PARAM_NAMES}

    def _render_lists(self, quantized):
        if quantized and self.qvalid and getattr(self, "_qrecon_lists", None) is not None:
            return self._qrecon_lists
        if not quantized and self.valid and getattr(self, "_recon_lists", None) is not None:
            return self._recon_lists
        return self._lists

    def _render_grid(self, m):
        shape, n = self.image.shape, self.batch_size_valued
        grid = [int(shape[l]) // n[l] for l in range(self.dim_domain)]
        extent = [g * ml for g, ml in zip(grid, m)]
        return grid, extent, [blk.render_axis(int(shape[l]), extent[l]) for l in range(self.dim_domain)]

    def _engine_render(self, params, lists, axes, m, grid, extent, out, tdt, want_argmax):
        return self._engine.render(params, lists, axes, m, first_batch=self.lo, out=out, dtype=tdt, want_argmax=want_argmax,
                                   num_batches=self.hi - self.lo)
