"""Held-out-view evaluation with the reference's names and file layout (volsurfs_py/utils/evaluation.py).

* `image_metrics` — per-image PSNR and SSIM of B views on the device, one HIP launch pair
  (vsa_image_metrics, csrc/image_metrics.hip); `psnr` / `ssim` are piq 0.8.0's call shapes on top of
  it, so `psnr(pred, gt, data_range=1.0)` of evaluation.py:167-168 ports unchanged.  piq itself is
  absent: the definitions are restated in DESIGN §13.
* `quantize_u8` — the 8-bit round trip the reference's scores go through (it writes PNGs and reads
  them back, rendering.py:15-33): u8 = trunc(clamp(x, 0, 1) * 255).  mvdatasets, which does this in
  the reference, is absent: the rule is a restatement, mirrored by `quantize8` in the kernel.
* `PerSceneEvaluator`, `render_and_eval`, `eval_rendered_imgs` — evaluation.py:15-83, :244-348 and
  :86-240: per-view and averaged CSVs, renders and ground truth as PNGs, in the reference's tree.
* `EvalCallback` — the `--eval_test / --eval_train` block of trainer.py:401-428 as a `trainer.train`
  callback.
LPIPS needs pretrained weights that do not exist offline: `lpips_fn` is the seam, and without it the
lpips column is nan.
"""
import csv
import os

import numpy as np
import torch

from . import _lib

_F32, _U8 = 0, 1


def pool_factor(H, W):
    """piq's SSIM downsampling factor: max(1, round(min(H, W) / 256)), Python's round (half to even)."""
    return max(1, round(min(int(H), int(W)) / 256))


def quantize_u8(img):
    """The 8-bit rule (PNG write): trunc(clamp(x, 0, 1) * 255) as a uint8 tensor on img's device.  The
    kernel's `quantize8` applies the same rule on load (image_metrics(..., quantize=True))."""
    if img.dtype == torch.uint8:
        return img
    return (img.float().clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def _dtype_flag(t, name):
    if t.dtype == torch.float32:
        return _F32
    if t.dtype == torch.uint8:
        return _U8
    raise ValueError(f"{name} must be float32 or uint8, got {t.dtype}")


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _check_pair(pred, gt):
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise ValueError("pred and gt must be tensors")
    if pred.shape != gt.shape:
        raise ValueError(f"pred and gt shapes differ: {tuple(pred.shape)} vs {tuple(gt.shape)}")
    if pred.dim() not in (3, 4) or pred.shape[-1] != 3:
        raise ValueError(f"expected [H,W,3] or [B,H,W,3] RGB images, got {tuple(pred.shape)}")
    if pred.dim() == 4 and pred.shape[0] < 1:
        raise ValueError("empty batch")
    _dtype_flag(pred, "pred")
    _dtype_flag(gt, "gt")


def _metrics(pred, gt, quantize, pool):
    """pred, gt: [B,H,W,3] float32 / uint8 -> (psnr [B] f64, ssim [B] f64) on the device."""
    B, H, W = pred.shape[0], pred.shape[1], pred.shape[2]
    if H // pool < 11 or W // pool < 11:
        raise ValueError(f"image {H}x{W} pooled by {pool} is {H // pool}x{W // pool}: SSIM's 11x11 kernel "
                         "needs at least 11x11")
    if not pred.is_cuda or not gt.is_cuda or pred.device != gt.device:
        raise ValueError("pred and gt must be on the same GPU")
    pf, gf = _dtype_flag(pred, "pred"), _dtype_flag(gt, "gt")
    fn = _lib.lib().vsa_image_metrics_workspace_bytes
    nbytes = int(fn(B, H, W, pool, pf, gf))
    if nbytes < 0:
        raise _lib.VolsurfsHipError(f"vsa_image_metrics_workspace_bytes failed with status {nbytes}")
    dev = pred.device
    with torch.cuda.device(dev):
        pred, gt = _aligned(pred), _aligned(gt)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        psnr = torch.empty(B, dtype=torch.float64, device=dev)
        ssim = torch.empty(B, dtype=torch.float64, device=dev)
        _lib.call("vsa_image_metrics", pred, pf, gt, gf, B, H, W, pool, int(bool(quantize) and pf == _F32),
                  ws, nbytes, psnr, ssim, _lib.stream_ptr())
    return psnr, ssim


def image_metrics(pred, gt, quantize=True):
    """PSNR and SSIM of each view: pred, gt [H,W,3] or [B,H,W,3], float32 (values in [0, 1]) or uint8 (read as
    u8 / 255), on the GPU.  quantize: an fp32 pred goes through the 8-bit rule first, as the reference's PNG round
    trip does (a uint8 pred already has).  -> {"psnr": [B] f64, "ssim": [B] f64}, on the device."""
    _check_pair(pred, gt)
    if pred.dim() == 3:
        pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
    psnr, ssim = _metrics(pred, gt, quantize, pool_factor(pred.shape[1], pred.shape[2]))
    return {"psnr": psnr, "ssim": ssim}


def _nchw_to_nhwc(x, y, data_range):
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise ValueError("x and y must be tensors")
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected two [N,3,H,W] tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dtype != y.dtype:
        raise ValueError(f"x and y dtypes differ: {x.dtype} vs {y.dtype}")
    if x.dtype == torch.uint8:
        if float(data_range) != 255.0:
            raise ValueError("uint8 inputs take data_range=255")
    else:
        if not x.is_floating_point():
            raise ValueError(f"unsupported dtype {x.dtype}")
        if float(data_range) != 1.0:
            raise ValueError("float inputs take data_range=1.0 (values in [0, 1])")
        x, y = x.float(), y.float()
    return x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()


_REDUCTIONS = ("none", "mean", "sum")


def _reduce(v, reduction):
    if reduction == "none":
        return v
    if reduction == "mean":
        return v.mean()
    return v.sum()


def psnr(x, y, data_range=1.0, reduction="mean", convert_to_greyscale=False):
    """piq.psnr on [N,3,H,W] (x: prediction, y: target): -10 log10(mse + 1e-8) per image.  (The images must be at
    least 11x11: the kernel computes SSIM alongside.)"""
    if convert_to_greyscale:
        raise ValueError("grey-scale PSNR is not supported")
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    xs, ys = _nchw_to_nhwc(x, y, data_range)
    return _reduce(_metrics(xs, ys, False, pool_factor(xs.shape[1], xs.shape[2]))[0], reduction)


def ssim(x, y, kernel_size=11, kernel_sigma=1.5, data_range=1.0, reduction="mean", full=False, downsample=True,
         k1=0.01, k2=0.03):
    """piq.ssim on [N,3,H,W] with piq's defaults (the only values the reference uses; others raise)."""
    if kernel_size != 11 or kernel_sigma != 1.5 or k1 != 0.01 or k2 != 0.03:
        raise ValueError("only piq's defaults are supported: kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03")
    if full:
        raise ValueError("full=True (the contrast-structure map) is not supported")
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    xs, ys = _nchw_to_nhwc(x, y, data_range)
    pool = pool_factor(xs.shape[1], xs.shape[2]) if downsample else 1
    return _reduce(_metrics(xs, ys, False, pool)[1], reduction)


class PerSceneEvaluator:
    """evaluation.py:15-83: per-image psnr / ssim / lpips of one render mode, their averages, and the CSV (one row
    per image, then an `avg` row; the reference builds a header row and never writes it)."""

    def __init__(self, render_mode):
        self.render_mode = render_mode
        self.imgs_results = {}

    def update(self, img_name, psnr, ssim, lpips):
        if img_name in self.imgs_results:
            print(f"WARNING: {img_name} already evaluated, overwriting")
        self.imgs_results[img_name] = {"psnr": psnr, "ssim": ssim, "lpips": lpips}

    def _avg(self, key):
        total = 0
        for res in self.imgs_results.values():
            total += res[key]
        return total / len(self.imgs_results)

    def psnr_avg(self):
        return self._avg("psnr")

    def ssim_avg(self):
        return self._avg("ssim")

    def lpips_avg(self):
        return self._avg("lpips")

    def results_averaged(self):
        return {"psnr": self.psnr_avg(), "ssim": self.ssim_avg(), "lpips": self.lpips_avg()}

    def save_to_csv(self, save_path, override_filename=None):
        name = override_filename if override_filename is not None else self.render_mode
        rows = [[k, r["psnr"], r["ssim"], r["lpips"]] for k, r in self.imgs_results.items()]
        avg = self.results_averaged()
        rows.append(["avg", avg["psnr"], avg["ssim"], avg["lpips"]])
        with open(os.path.join(save_path, f"{name}.csv"), "w") as f:
            csv.writer(f).writerows(rows)
        return rows


def _default_render_fn(method):
    from .renderers import BaseRenderer
    if isinstance(method, BaseRenderer):
        from .camera import get_camera_rays

        def render(cam):
            rays_o, rays_d, _ = get_camera_rays(cam)
            rgb = method.render_rays(rays_o, rays_d)["renders"]["ray_traced"]["rgb"]
            return rgb.reshape(cam.height, cam.width, 3)
        return render
    return lambda cam: method.render_camera(cam)["rgb"]


def _raytracer_of(method):
    rt = getattr(method, "raytracer", None)
    if rt is None and getattr(method, "method", None) is not None:    # a renderer around a VolSurfs
        rt = getattr(method.method, "raytracer", None)
    return rt


def _save_png(img_u8, path):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(img_u8.cpu().numpy()).save(path)


def _score(evaluator, names, preds, gts, batch, lpips_fn):
    """preds, gts: lists of [H,W,3] uint8 device tensors; scored in batches of `batch` views of one size."""
    i = 0
    while i < len(preds):
        j = i + 1
        while j < len(preds) and j - i < batch and preds[j].shape == preds[i].shape:
            j += 1
        res = image_metrics(torch.stack(preds[i:j]), torch.stack(gts[i:j]), quantize=False)
        p, s = res["psnr"].tolist(), res["ssim"].tolist()
        for k in range(i, j):
            lp = float("nan")
            if lpips_fn is not None:
                lp = float(lpips_fn(preds[k].permute(2, 0, 1)[None].float() / 255.0,
                                    gts[k].permute(2, 0, 1)[None].float() / 255.0))
            evaluator.update(names[k], p[k - i], s[k - i], lp)
        i = j


@torch.no_grad()
def render_and_eval(method, splits, save_path=None, iter_nr=None, save_pngs=True, lpips_fn=None, render_fn=None,
                    batch=16):
    """evaluation.py:244-348: render every view of every split on the device, quantise it to 8 bits, score it
    against its ground truth and return {split: {"psnr", "ssim", "lpips"}} (the averages).

    splits: {name: (cameras, rgbs)} with rgbs [C,H,W,3] float32 or uint8 (the pair a TensorReel is built from).
    method: a VolSurfs (method.render_camera(cam)["rgb"]) or a renderers.BaseRenderer such as VolsurfsRenderer
    (render_rays(...)["renders"]["ray_traced"]["rgb"]); render_fn(cam) -> [H,W,3] replaces either.
    save_path: write <save_path>/<iter:07d>/renders/<split>/ray_traced/{rgb,gt}/<idx:03d>.png (save_pngs),
    .../renders/<split>/ray_traced.csv and <save_path>/results/<split>.csv.
    The ray tracer's feedback buffer is the object it was on entry when this returns: a captured GraphTrainLoop
    holds its raw pointer, and a render of more rays than the training batch would replace it."""
    render = render_fn or _default_render_fn(method)
    rt = _raytracer_of(method)
    fb = rt._fb if rt is not None else None
    out = {}
    try:
        for split, (cameras, rgbs) in splits.items():
            if len(cameras) != len(rgbs):
                raise ValueError(f"split {split!r}: {len(cameras)} cameras but {len(rgbs)} images")
            names, preds, gts = [], [], []
            for idx, cam in enumerate(cameras):
                pred = quantize_u8(render(cam))
                gt = torch.as_tensor(rgbs[idx])
                gt = quantize_u8(gt.to(pred.device))
                if tuple(pred.shape) != (cam.height, cam.width, 3) or gt.shape != pred.shape:
                    raise ValueError(f"split {split!r} view {idx}: render {tuple(pred.shape)}, "
                                     f"ground truth {tuple(gt.shape)}, camera {cam.height}x{cam.width}")
                names.append(format(idx, "03d"))
                preds.append(pred)
                gts.append(gt)
            ev = PerSceneEvaluator("ray_traced")
            _score(ev, names, preds, gts, batch, lpips_fn)
            out[split] = ev.results_averaged()
            if save_path is not None:
                renders = os.path.join(save_path, format(iter_nr or 0, "07d"), "renders", split)
                os.makedirs(renders, exist_ok=True)
                if save_pngs:
                    for name, p, g in zip(names, preds, gts):
                        _save_png(p, os.path.join(renders, "ray_traced", "rgb", name + ".png"))
                        _save_png(g, os.path.join(renders, "ray_traced", "gt", name + ".png"))
                ev.save_to_csv(renders)
                results = os.path.join(save_path, "results")
                os.makedirs(results, exist_ok=True)
                ev.save_to_csv(results, override_filename=split)
    finally:
        if rt is not None:
            rt._fb = fb
    return out


def _read_png_u8(path):
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im.convert("RGB"))           # a writable copy
    return torch.from_numpy(a)


@torch.no_grad()
def eval_rendered_imgs(renders_path, lpips_fn=None, device="cuda"):
    """evaluation.py:86-240: score a renders/<split> tree offline.  Every folder of renders_path with `gt` and `rgb`
    subfolders is a render mode; its PNGs are scored pairwise by file name.  -> [PerSceneEvaluator], one per render
    mode (folders in sorted order)."""
    if not os.path.isdir(renders_path):
        raise FileNotFoundError(f"renders path {renders_path} for evaluation does not exist")
    results = []
    for mode in sorted(os.listdir(renders_path)):
        mode_path = os.path.join(renders_path, mode)
        gt_dir, rgb_dir = os.path.join(mode_path, "gt"), os.path.join(mode_path, "rgb")
        if not (os.path.isdir(gt_dir) and os.path.isdir(rgb_dir)):
            continue
        files = sorted(os.listdir(gt_dir))
        ev = PerSceneEvaluator(mode)
        names, preds, gts = [], [], []
        for fn in files:
            names.append(fn.split(".")[0])
            gts.append(_read_png_u8(os.path.join(gt_dir, fn)).to(device))
            preds.append(_read_png_u8(os.path.join(rgb_dir, fn)).to(device))
        _score(ev, names, preds, gts, 1, lpips_fn)
        results.append(ev)
    return results


class EvalCallback:
    """trainer.train callback: render_and_eval(method, splits, ...) at iter_ended when (phase.iter_nr + 1) % every
    == 0, and at training_ended unless that last iteration was just evaluated.  The reference's condition,
    `phase.iter_nr + 1 % eval_test_freq == 0` (trainer.py:407,416), parses as iter_nr + (1 % freq) and so fires only
    at the last iteration; this is the periodic rule it means.  `method` is what trainer.train trains (its hooks do
    not hand it over); the other keywords go to render_and_eval.  callback.history: [(iter_nr, results)]."""

    def __init__(self, splits, every, save_path=None, *, method, **render_and_eval_kw):
        if int(every) < 1:
            raise ValueError("every must be >= 1")
        self.method, self.splits, self.every = method, splits, int(every)
        self.save_path, self.kw = save_path, render_and_eval_kw
        self.history = []
        self._last_iter = None

    def _eval(self, iter_nr):
        res = render_and_eval(self.method, self.splits, save_path=self.save_path, iter_nr=iter_nr, **self.kw)
        self.history.append((iter_nr, res))

    def iter_ended(self, phase, **kw):
        self._last_iter = phase.iter_nr
        if (phase.iter_nr + 1) % self.every == 0:
            self._eval(phase.iter_nr)

    def training_ended(self, **kw):
        if self._last_iter is not None and (not self.history or self.history[-1][0] != self._last_iter):
            self._eval(self._last_iter)


__all__ = ["pool_factor", "quantize_u8", "image_metrics", "psnr", "ssim", "PerSceneEvaluator", "render_and_eval",
           "eval_rendered_imgs", "EvalCallback"]
