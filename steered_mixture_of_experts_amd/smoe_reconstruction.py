"""Decode-side entry point (reference smoe_reconstruction.py:15-79): parameter pickle ->
``Smoe(init_params=...)`` -> ONE forward pass -> reconstructed image.

    python -m steered_mixture_of_experts_amd.smoe_reconstruction -i IMG -r OUT -p params.pkl

``--scale S`` (one value or one per axis) / ``--frames F`` (samples per block on the time axis of video input) decode the
model on another sampling grid with ``Smoe.render`` / ``SharedSmoe.render`` (per-block and whole-image pickles alike; on
the device, written straight into the stitched image); with the defaults the output is the reference's.
``--blend B`` (source pixels, one value or one per axis; per-block models only) cross-fades neighbouring blocks within ``B``
pixels of every block border (``Smoe.render(blend=...)``): no block seams in the enlarged image.
``--window LO HI ...`` (two numbers per axis, source pixels) and / or ``--size E ...`` (output samples per axis) decode a
viewport with ``Smoe.render_view``: only that window of the image, at that size (``--size`` absent: ``--scale`` times the
window; ``--window`` absent: the whole image); they work together with ``--scale`` and ``--blend``; per-block models only.
``--affine M.. T..`` (``d (d + 1)`` numbers, row-major ``[M | t]``) with ``--size`` decodes an affine view with
``Smoe.render_warp``: output cell centre ``i + 0.5`` shows the source position ``M (i + 0.5) + t`` (source pixels), a rotation
or a shear included; it works with ``--blend``, not with ``--window`` / ``--frames`` / ``--scale``; per-block models only.
``--taps N ...`` (one number or one per axis) or ``--taps auto`` with ``--affine`` or ``--window`` / ``--size`` averages every
output sample over that many taps per axis inside its cell (``Smoe.sample_area``): a view coarser than the source that does
not alias; per-block models only.
``--homography H..`` (``(d + 1)^2`` numbers, row-major) with ``--size`` decodes a projective view with
``Smoe.render_projective``: output cell centre ``c = i + 0.5`` shows the source position ``(H[:d, :d] c + H[:d, d]) / (H[d, :d] .
c + H[d, d])``, every sample averaged over its OWN footprint (``Smoe.sample_area_each``; ``--taps`` defaults to ``auto`` here);
samples behind the horizon are 0; it works with ``--blend``, not with ``--affine`` / ``--window`` / ``--frames`` / ``--scale``;
per-block models only.
"""
import argparse
import os
import re

import numpy as np

from . import blocks as blk
from .smoe import SharedSmoe, Smoe
from .utils import load_checkpoint, read_image, write_image


def _decode_batch_shape(image_shape, channels, batches):
    """Batch shape for decoding a whole-image (shared-kernel) model: the reference's divisor search
    (smoe.py:2459-2543) with the smallest batch count >= ``batches`` whose batches fit the kernels' LDS tile.  Every
    batch lists every kernel at the start (smoe.py:315), so the split does not change the reconstruction."""
    limit = 2048 if channels == 1 else 1024
    d = len(image_shape)
    n = max(1, int(batches))
    total = int(np.prod(image_shape))
    while n <= total:
        bs = blk.get_batch_shape(n, tuple(image_shape) + (d + channels,))[:-1]
        if int(np.prod(bs)) <= limit:
            return [int(b) for b in bs]
        n = int(np.prod([s // b for s, b in zip(image_shape, bs)])) + 1
    raise ValueError("no batch shape fits")


_shared_engine_factory = None      # tests put the oracle-backed engine here; None = the HIP engine


def main(image_path, results_path, params_file, batches=1, bit_depths=(20, 18, 6, 10, 10), quant_params=False,
         scale=None, frames=None, blend=None, window=None, size=None, affine=None, taps=None, homography=None):
    if len(bit_depths) != 5:
        raise ValueError("Number of bit depths must be five!")           # smoe_reconstruction.py:17-18
    orig, precision, _ = read_image(image_path)
    cp = load_checkpoint(params_file)
    init_params = cp['params']
    tp = _taps_option(taps)
    if tp is not None:
        if np.asarray(init_params['pis']).ndim == 1:
            raise ValueError("--taps needs a per-block model: this pickle holds a whole-image (shared-kernel) model, which "
                             "has no area-averaged decoder")
        if affine is None and window is None and size is None and homography is None:
            raise ValueError("--taps needs --affine or --window / --size (the view whose cells are averaged)")
    if results_path is not None and not os.path.exists(results_path):
        os.mkdir(results_path)
    # the graph the model was trained on (smoe_reconstruction.py:32-43 copies these from the pickle onto the model; here
    # they go through the constructor so that the kernels are built for them).  Absent keys keep the defaults.
    qmode = int(cp.get('quantization_mode') or 0)
    common = dict(init_params=init_params, bit_depths=list(bit_depths), precision=precision,
                  use_determinant=bool(cp.get('use_determinant', True)), use_yuv=bool(cp.get('use_yuv', False)),
                  train_inverse_cov=bool(cp.get('train_inverse_cov', False)),    # absent key: trained by the CLI (False)
                  radial_as=bool(cp.get('radial_as', False)), quantization_mode=qmode,
                  quantize_pis=bool(cp.get('quantized_pis', False)))
    for key in ('lower_bounds', 'upper_bounds'):
        if cp.get(key) is not None:
            common[key] = list(cp[key])
    if np.asarray(init_params['pis']).ndim == 1:
        # ONE model for the whole image = the reference's own checkpoint layout (utils.save_model, kernels leading;
        # with reduce=True only the kernels with pis > 0) and this package's --mode shared pickles
        d = orig.ndim - 1
        bs = cp.get('batch_size') or _decode_batch_shape(orig.shape[:d], orig.shape[-1], batches)
        smoe = SharedSmoe(orig, batch_size=list(bs), only_y_gamma=bool(cp.get('only_y_gamma', False)),
                          use_diff_center=False, engine_factory=_shared_engine_factory, **common)
    else:
        smoe = Smoe(orig, start_batches=batches, batch_size=list(cp['batch_size']), **common)
    with_q = bool(quant_params) and smoe.quantization_mode <= 0         # smoe_reconstruction.py:46-51
    if with_q:
        from .quantizer import quantize_params, rescaler
        smoe.qparams = quantize_params(smoe, smoe.get_params())
        smoe.rparams = rescaler(smoe, smoe.qparams)
    loss, mse, _, _ = smoe.run_batched(train=False, update_reconstruction=True, with_quantized_params=with_q)
    found = re.findall(r'\d+', os.path.basename(params_file))
    iter_str = found[-1] if found else "0"
    reconstruction_path = results_path + '/' + iter_str + "_reconstruction"
    if with_q:                                                          # smoe_reconstruction.py:58-75
        reconstruction = smoe.get_qreconstruction()
        reconstruction_path += "_{0:1d}_{1:1d}_{2:1d}_{3:1d}_{4:1d}".format(*bit_depths)
    else:
        reconstruction = smoe.get_reconstruction()
    sc = [float(v) for v in np.atleast_1d(1.0 if scale is None else scale)]
    bl = [float(v) for v in np.atleast_1d(0.0 if blend is None else blend)]
    if homography is not None:
        # a projective view: every output sample at its own source position, averaged over its own footprint
        # (Smoe.render_projective)
        if not hasattr(smoe, "render_projective"):
            raise ValueError("--homography needs a per-block model: this pickle holds a whole-image (shared-kernel) model, "
                             "which has no point decoder")
        d = smoe.dim_domain
        if size is None:
            raise ValueError("--homography needs --size (the output samples per axis)")
        if affine is not None or window is not None or frames is not None or scale is not None:
            raise ValueError("--homography does not go with --affine / --window / --frames / --scale (the matrix holds them)")
        if len(homography) != (d + 1) * (d + 1):
            raise ValueError(f"--homography takes {(d + 1) * (d + 1)} numbers: the rows of H")
        if len(size) != d:
            raise ValueError(f"--size takes one number per axis ({d})")
        tph = "auto" if tp is None else tp
        reconstruction = smoe.render_projective(np.asarray(homography, dtype=np.float64).reshape(d + 1, d + 1),
                                                [int(v) for v in size], taps=tph, quantized=with_q, blend=bl)
        reconstruction_path += "_proj" + "x".join(str(v) for v in reconstruction.shape[:d]) + _taps_suffix(tph)
        if any(v != 0.0 for v in bl):
            reconstruction_path += "_blend" + "x".join("%g" % v for v in bl)
    elif affine is not None:
        # an affine view: every output sample at its own source position (Smoe.render_warp)
        if not hasattr(smoe, "render_warp"):
            raise ValueError("--affine needs a per-block model: this pickle holds a whole-image (shared-kernel) model, which "
                             "has no point decoder")
        d = smoe.dim_domain
        if size is None:
            raise ValueError("--affine needs --size (the output samples per axis)")
        if window is not None or frames is not None or scale is not None:
            raise ValueError("--affine does not go with --window / --frames / --scale (the matrix holds them)")
        if len(affine) != d * (d + 1):
            raise ValueError(f"--affine takes {d * (d + 1)} numbers: the rows of [M | t]")
        if len(size) != d:
            raise ValueError(f"--size takes one number per axis ({d})")
        reconstruction = smoe.render_warp(np.asarray(affine, dtype=np.float64).reshape(d, d + 1), [int(v) for v in size],
                                          quantized=with_q, blend=bl, taps=tp)
        reconstruction_path += "_warp" + "x".join(str(v) for v in reconstruction.shape[:d]) + _taps_suffix(tp)
        if any(v != 0.0 for v in bl):
            reconstruction_path += "_blend" + "x".join("%g" % v for v in bl)
    elif window is not None or size is not None:
        # a viewport: that window of the image at that size and nothing else (Smoe.render_view)
        if not hasattr(smoe, "render_view"):
            raise ValueError("--window / --size need a per-block model: this pickle holds a whole-image (shared-kernel) "
                             "model, which has no viewport decoder")
        d = smoe.dim_domain
        if frames is not None:
            raise ValueError("--frames does not go with --window / --size (give the time axis its own window and size)")
        if window is not None and len(window) != 2 * d:
            raise ValueError(f"--window takes two numbers per axis ({2 * d})")
        if size is not None and len(size) != d:
            raise ValueError(f"--size takes one number per axis ({d})")
        if size is not None and scale is not None:
            raise ValueError("--size and --scale both set the output size: give one")
        if len(sc) not in (1, d):
            raise ValueError(f"--scale takes one value or {d}")
        win = None if window is None else [(float(window[2 * l]), float(window[2 * l + 1])) for l in range(d)]
        reconstruction = smoe.render_view(win, size=None if size is None else [int(v) for v in size],
                                          scale=None if size is not None else sc, quantized=with_q, blend=bl, taps=tp)
        reconstruction_path += "_view" + "x".join(str(v) for v in reconstruction.shape[:d]) + _taps_suffix(tp)
        if any(v != 0.0 for v in bl):
            reconstruction_path += "_blend" + "x".join("%g" % v for v in bl)
    elif frames is not None or any(v != 1.0 for v in sc) or any(v != 0.0 for v in bl):
        # another sampling grid: evaluate the model there (Smoe.render / SharedSmoe.render); the pass above keeps loss / mse
        # as reported
        d = smoe.dim_domain
        sc = sc * d if len(sc) == 1 else sc
        if len(sc) != d:
            raise ValueError(f"--scale takes one value or {d}")
        if frames is not None and d != 3:
            raise ValueError("--frames needs video input")
        m = [max(1, int(round(v * n))) for v, n in zip(sc, smoe.batch_size_valued)]
        if frames is not None:
            m[2] = int(frames)
        reconstruction = smoe.render(samples_per_block=m, quantized=with_q, blend=bl)
        reconstruction_path += "_" + "x".join(str(v) for v in m)
        if any(v != 0.0 for v in bl):
            reconstruction_path += "_blend" + "x".join("%g" % v for v in bl)
    write_image(reconstruction, reconstruction_path, smoe.dim_domain, smoe.use_yuv, precision)
    return reconstruction, loss, mse


def _taps_option(taps):
    """``--taps``: None, ``"auto"`` or a list of ints"""
    if taps is None:
        return None
    vals = [taps] if isinstance(taps, (str, int)) else list(taps)
    if len(vals) == 1 and str(vals[0]) == "auto":
        return "auto"
    try:
        return [int(v) for v in vals]
    except (TypeError, ValueError):
        raise ValueError("--taps takes auto, one number or one per axis") from None


def _taps_suffix(tp):
    if tp is None:
        return ""
    return "_taps" + ("auto" if tp == "auto" else "x".join(str(v) for v in tp))


def _parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('-i', '--image_path', type=str, required=True, help="input image")
    parser.add_argument('-r', '--results_path', type=str, required=True, help="results path")
    parser.add_argument('-p', '--params_file', type=str, required=True, help="parameter file for model initialization.")
    parser.add_argument('-b', '--batches', type=int, default=1)
    parser.add_argument('-bd', '--bit_depths', type=int, default=[20, 18, 6, 10, 10], nargs='+')
    parser.add_argument('-qp', '--quant_params', action='store_true')
    parser.add_argument('--scale', type=float, default=None, nargs='+',
                        help="render at this scale (one value or one per axis; default 1 = the training lattice)")
    parser.add_argument('--frames', type=int, default=None, help="video: samples per block on the time axis")
    parser.add_argument('--blend', type=float, default=None, nargs='+',
                        help="cross-fade neighbouring blocks within this many source pixels of a block border (one value or "
                             "one per axis, at most half a block; default 0 = off; per-block models only)")
    parser.add_argument('--window', type=float, default=None, nargs='+',
                        help="decode only this window of the image: LO HI per axis, in source pixels (per-block models only)")
    parser.add_argument('--size', type=int, default=None, nargs='+',
                        help="output samples per axis of the window (default: --scale times the window)")
    parser.add_argument('--affine', type=float, default=None, nargs='+',
                        help="decode an affine view of --size samples: the d (d + 1) numbers of [M | t], row-major; output "
                             "cell centre i + 0.5 shows source position M (i + 0.5) + t (per-block models only)")
    parser.add_argument('--homography', type=float, default=None, nargs='+',
                        help="decode a projective view of --size samples: the (d + 1)^2 numbers of H, row-major; output cell "
                             "centre c = i + 0.5 shows source position (H[:d,:d] c + H[:d,d]) / (H[d,:d] . c + H[d,d]), averaged "
                             "over its own footprint (--taps, default auto; per-block models only)")
    parser.add_argument('--taps', type=str, default=None, nargs='+',
                        help="with --affine, --homography or --window / --size: average every output sample over this many taps per axis "
                             "inside its cell (one number, one per axis, or auto = one per source pixel covered; 1 .. 16 each, "
                             "at most 64 in all; per-block models only)")
    return parser


def _cli(argv=None):
    args = _parser().parse_args(argv)
    main(**vars(args))


if __name__ == '__main__':
    _cli()
