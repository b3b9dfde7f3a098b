"""Scenes from disk: the cameras and images of a Blender-format (`blender`, `blendernerf`, `shelly`) or a DTU (NeuS / IDR
layout) scene, prepared for every stage of this library.

The reference gets them from `mvdatasets.MVDataset(dataset, scene, path, splits, config)` (trainer.py:570-593, baker.py:
281-301, utils/volsurfs_utils.py:234-272), an empty submodule in its checkout: the formats are public, the rules below are
this library's own, restated in tests/datasets_restated.py and UNPINNED.

* `read_blender_split`, `read_dtu_scene` — host parsers (numpy only): intrinsics, camera-to-world poses and file lists.
* `DataParams` — a dataset's settings, overridden per scene (params/data_params.py).
* `MVDataset` / `DataCamera` — the loaded scene: `mv[split]` cameras, `images(split)` / `masks(split)` device stacks
  made from the decoded bytes by one `vsa_images_prepare` launch per split (csrc/image_prepare.hip), `splits(names)` for
  `render_and_eval` / `EvalCallback`, `reel(split)` for training.
* `init_bounding_primitive` — utils/volsurfs_utils.py:234-272.
* `write_blender_scene`, `write_dtu_scene` — the inverses of the two parsers.

Decoding PNGs (PIL, a thread pool on the host) dominates a load; the kernel is a small bandwidth-bound pass behind it.
"""
import ctypes
import json
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .background import BoundingBox, BoundingSphere
from .camera import Camera, TensorReel
from .texture_export import FAR, NEAR, _FLIP_YZ, _bg_color_of, opengl_camera

BLENDER_FAMILY = ("blender", "blendernerf", "shelly")
DATASETS = BLENDER_FAMILY + ("dtu",)
MAX_SUBSAMPLE = 16
_DECODE_THREADS = 16


def opengl_to_camera(matrix_world):
    """A 4x4 OpenGL camera matrix (x right, y up, z back) as a `camera.Camera` pose (x right, y down, z forward), and
    back: matrix . diag(1, -1, -1, 1), the `matrixWorld` rule of `texture_export.opengl_camera` (its own inverse)."""
    return np.asarray(matrix_world, np.float64) @ _FLIP_YZ


# ---------------------------------------------------------------------------------------------------------- parsers

def _image_size(path):
    from PIL import Image
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    with Image.open(path) as im:          # reads the header only
        return im.size[1], im.size[0]


def _resolve_image(scene_dir, file_path):
    path = os.path.normpath(os.path.join(scene_dir, file_path))
    for p in (path, path + ".png"):
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"{path} (nor {path}.png)")


def read_blender_split(scene_dir, split, test_skip=1):
    """`transforms_<split>.json` of a Blender-format scene -> {intrinsics [n,3,3] f64, c2w [n,4,4] f64, image_paths,
    mask_paths (None: the masks are the images' alpha), height, width, index}.
    Frames in file order; for split "test" only, every `test_skip`-th one from 0 (`index` keeps the position in the
    file).  `file_path` is resolved against `scene_dir` as written, then with ".png" appended.  H, W from the first
    image's header; fx = fy = 0.5 W / tan(0.5 camera_angle_x) in fp64, cx = 0.5 W, cy = 0.5 H;
    c2w = transform_matrix . diag(1, -1, -1, 1) (`opengl_to_camera`)."""
    test_skip = int(test_skip)
    if test_skip < 1:
        raise ValueError(f"test_skip must be >= 1, got {test_skip}")
    path = os.path.join(scene_dir, f"transforms_{split}.json")
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    with open(path) as f:
        meta = json.load(f)
    frames = meta["frames"]
    index = list(range(len(frames)))
    if split == "test":
        index = index[::test_skip]
    if not index:
        raise ValueError(f"{path}: no frames")
    image_paths = [_resolve_image(scene_dir, frames[i]["file_path"]) for i in index]
    H, W = _image_size(image_paths[0])
    fx = 0.5 * W / math.tan(0.5 * float(meta["camera_angle_x"]))
    K = np.array([[fx, 0.0, 0.5 * W], [0.0, fx, 0.5 * H], [0.0, 0.0, 1.0]])
    c2w = np.stack([opengl_to_camera(np.asarray(frames[i]["transform_matrix"], np.float64).reshape(4, 4))
                    for i in index])
    return {"intrinsics": np.repeat(K[None], len(index), 0), "c2w": c2w, "image_paths": image_paths,
            "mask_paths": None, "height": H, "width": W, "index": index}


def decompose_projection(P):
    """A 3x4 projection P ~ K [R | -R c] -> (K [3,3] with a positive diagonal and K[2,2] = 1, R [3,3] world-to-camera
    with det +1, c [3] the centre), in fp64: P is negated when det(P[:, :3]) < 0, then RQ-decomposed."""
    P = np.asarray(P, np.float64)[:3, :4]
    if np.linalg.det(P[:, :3]) < 0:
        P = -P
    M = P[:, :3]
    # RQ from numpy's QR: with J the row reversal, (J M)^T = Q' R' gives M = (J R'^T J) (J Q'^T)
    q, r = np.linalg.qr(M[::-1].T)
    K, R = r.T[::-1, ::-1], q.T[::-1]
    S = np.diag(np.where(np.diag(K) < 0, -1.0, 1.0))
    K, R = K @ S, S @ R
    c = -np.linalg.solve(M, P[:, 3])
    return K / K[2, 2], R, c


def _sorted_files(d):
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))]


def read_dtu_scene(scene_dir):
    """A DTU scene in the NeuS / IDR layout -> the dict of `read_blender_split` for ALL of its n views (`MVDataset` splits
    them).  Cameras from `cameras_sphere.npz`, else `cameras.npz`: P = (world_mat_i . scale_mat_i)[:3, :4],
    `decompose_projection`, c2w = [R^T | c] (so the object sits in the unit sphere scale_mat normalised it to).  Images:
    the sorted files of `image/`; masks: those of `mask/` if it exists; both paired with the cameras by position, and a
    count that is not n raises ValueError."""
    for name in ("cameras_sphere.npz", "cameras.npz"):
        path = os.path.join(scene_dir, name)
        if os.path.isfile(path):
            break
    else:
        raise FileNotFoundError(os.path.join(scene_dir, "cameras_sphere.npz"))
    with np.load(path) as z:
        n = 0
        while f"world_mat_{n}" in z.files:
            n += 1
        if n == 0:
            raise ValueError(f"{path}: no world_mat_0")
        Ks, poses = [], []
        for i in range(n):
            world = np.asarray(z[f"world_mat_{i}"], np.float64)
            scale = np.asarray(z[f"scale_mat_{i}"], np.float64) if f"scale_mat_{i}" in z.files else np.eye(4)
            K, R, c = decompose_projection((world @ scale)[:3, :4])
            pose = np.eye(4)
            pose[:3, :3], pose[:3, 3] = R.T, c
            Ks.append(K)
            poses.append(pose)
    image_dir, mask_dir = os.path.join(scene_dir, "image"), os.path.join(scene_dir, "mask")
    if not os.path.isdir(image_dir):
        raise FileNotFoundError(image_dir)
    image_paths = _sorted_files(image_dir)
    mask_paths = _sorted_files(mask_dir) if os.path.isdir(mask_dir) else None
    if len(image_paths) != n:
        raise ValueError(f"{scene_dir}: {n} cameras but {len(image_paths)} images")
    if mask_paths is not None and len(mask_paths) != n:
        raise ValueError(f"{scene_dir}: {n} cameras but {len(mask_paths)} masks")
    H, W = _image_size(image_paths[0])
    return {"intrinsics": np.stack(Ks), "c2w": np.stack(poses), "image_paths": image_paths, "mask_paths": mask_paths,
            "height": H, "width": W, "index": list(range(n))}


def _take(rec, keep):
    return {"intrinsics": rec["intrinsics"][keep], "c2w": rec["c2w"][keep],
            "image_paths": [rec["image_paths"][i] for i in keep],
            "mask_paths": None if rec["mask_paths"] is None else [rec["mask_paths"][i] for i in keep],
            "height": rec["height"], "width": rec["width"], "index": [rec["index"][i] for i in keep]}


# ----------------------------------------------------------------------------------------------------------- params

def _as_factor(v):
    if float(v) != int(v):
        raise ValueError(f"subsample_factor must be an integer, got {v!r}")
    return int(v)


def _as_bg(v):
    return v if v is None or isinstance(v, str) else tuple(float(x) for x in v)


def _opt_float(v):
    return None if v is None else float(v)


# the keys of params/data_params.py:45-95 and their types
_KEYS = {"bg_color": _as_bg, "subsample_factor": _as_factor, "scene_radius_mult": float, "load_mask": bool,
         "target_cameras_max_distance": _opt_float, "rotate_scene_x_axis_deg": float, "translate_scene_x": float,
         "translate_scene_y": float, "translate_scene_z": float, "train_test_overlap": bool,
         "test_camera_freq": int, "white_bg": bool, "test_skip": int, "init_sphere_scale": float,
         "scene_type": str}
_DEFAULTS = {"bg_color": None, "subsample_factor": 1, "scene_radius_mult": 1.0, "load_mask": True,
             "target_cameras_max_distance": None, "rotate_scene_x_axis_deg": 0.0, "translate_scene_x": 0.0,
             "translate_scene_y": 0.0, "translate_scene_z": 0.0, "train_test_overlap": False, "test_camera_freq": 8,
             "white_bg": False, "test_skip": 1, "init_sphere_scale": 0.5, "scene_type": "bounded"}
# nerf_synthetic's geometry: cameras on an orbit of radius 4.03 around an object within +-1.5, so with the orbit scaled
# to 1 the object fits a radius of 0.5 with a third to spare.  Chosen from that geometry, NOT verified against data.
_BLENDER_DEFAULTS = {"target_cameras_max_distance": 1.0, "scene_radius_mult": 0.5}


class DataParams:
    """The settings of one scene: the defaults, overridden by `cfg[dataset_name]`'s keys, overridden by
    `cfg[dataset_name]["scenes"][scene_name]`'s (params/data_params.py; `cfg` is the parsed data config, a dict).  Each
    key is an attribute; `.dict()` gives them all.  A dataset that `cfg` does not name gets the defaults: those of the
    table in DESIGN §30, with the Blender family's camera distance of 1 and radius multiplier of 0.5 (chosen from
    nerf_synthetic's geometry, an orbit at 4.03 around an object within +-1.5; unverified against data)."""

    def __init__(self, dataset_name, scene_name, cfg=None):
        self.dataset_name, self.scene_name = dataset_name, scene_name
        values = dict(_DEFAULTS)
        if dataset_name in BLENDER_FAMILY:
            values.update(_BLENDER_DEFAULTS)
        ds = dict((cfg or {}).get(dataset_name) or {})
        ds.update((ds.pop("scenes", None) or {}).get(scene_name) or {})
        for key, value in ds.items():
            if key in _KEYS:
                values[key] = _KEYS[key](value)
        if values["scene_type"] not in ("bounded", "unbounded"):
            raise ValueError(f"scene_type must be 'bounded' or 'unbounded', got {values['scene_type']!r}")
        if not 1 <= values["subsample_factor"] <= MAX_SUBSAMPLE:
            raise ValueError(f"subsample_factor must be in 1..{MAX_SUBSAMPLE}, got {values['subsample_factor']}")
        if values["test_skip"] < 1 or values["test_camera_freq"] < 1:
            raise ValueError("test_skip and test_camera_freq must be >= 1")
        self._values = values
        for key, value in values.items():
            setattr(self, key, value)

    def dict(self):
        return dict(self._values)

    def background(self):
        """The colour images are composited over: `bg_color` ("white", "black" or a triple), else white with
        `white_bg`, else black.  "random" raises: a loader must be repeatable."""
        bg = self.bg_color
        if bg is None:
            bg = "white" if self.white_bg else "black"
        if bg == "random":
            raise ValueError("bg_color 'random': a loader must be repeatable (give 'white', 'black' or a colour)")
        try:
            return tuple(float(v) for v in _bg_color_of(bg))
        except _lib.VolsurfsHipError as e:
            raise ValueError(f"bg_color: {e}") from None


def transform_poses(c2w_by_split, params):
    """The scene transforms of `params` on fp64 camera-to-world poses {split: [n,4,4]}, in this order: rotate the world
    about x by `rotate_scene_x_axis_deg`, translate by `translate_scene_x/y/z`, scale the centres by
    `target_cameras_max_distance` / max_i |c_i| (the maximum over all the splits given, so that they share one frame;
    None: no scaling).  Returns ({split: [n,4,4]}, the scale applied)."""
    a = math.radians(params.rotate_scene_x_axis_deg)
    rot = np.eye(4)
    rot[1:3, 1:3] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    shift = np.array([params.translate_scene_x, params.translate_scene_y, params.translate_scene_z])
    out = {}
    for split, c2w in c2w_by_split.items():
        c2w = np.asarray(c2w, np.float64)
        if params.rotate_scene_x_axis_deg != 0.0:
            c2w = rot @ c2w
        c2w = c2w.copy()
        c2w[:, :3, 3] += shift
        out[split] = c2w
    scale = 1.0
    if params.target_cameras_max_distance is not None:
        far = max(float(np.linalg.norm(c2w[:, :3, 3], axis=1).max()) for c2w in out.values())
        if not far > 0.0:
            raise ValueError("target_cameras_max_distance: every camera is at the origin")
        scale = params.target_cameras_max_distance / far
        for c2w in out.values():
            c2w[:, :3, 3] *= scale
    return out, scale


# ---------------------------------------------------------------------------------------------------------- images

def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGBA", "RGB", "L"):
            im = im.convert("RGBA")
        a = np.asarray(im)
    return a[..., None] if a.ndim == 2 else a


def _decode_mask(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im if im.mode == "L" else im.convert("L"))


def _decode_stack(paths, decode, what):
    """[n, H, W, ch] u8 of the files, decoded in a thread pool; one size and one channel count, else ValueError."""
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(p)
    with ThreadPoolExecutor(min(_DECODE_THREADS, os.cpu_count() or 1)) as pool:
        arrays = list(pool.map(decode, paths))
    for p, a in zip(paths, arrays):
        if a.shape != arrays[0].shape:
            raise ValueError(f"{what}: {p} is {a.shape}, {paths[0]} is {arrays[0].shape}: one split holds one size "
                             "and one channel count")
    return np.stack(arrays)


def prepare_images(src, mask=None, subsample_factor=1, bg=(0.0, 0.0, 0.0)):
    """(rgb [C,H,W,3] f32, mask [C,H,W] f32 or None) from src [C,H0,W0,ch] u8 (ch 1, 3 or 4) and mask [C,H0,W0] u8 or
    None, both cuda: alpha over `bg`, box subsampling and the mask in one `vsa_images_prepare` launch (the rule: include/
    volsurfs_hip.h "Image preparation").  The mask is `mask`'s when given, else the alpha channel's, else None."""
    if src.dtype != torch.uint8 or src.dim() != 4 or not src.is_cuda or not src.is_contiguous():
        raise _lib.VolsurfsHipError(f"prepare_images: src must be a contiguous cuda uint8 [C,H,W,ch], got {src.dtype} "
                                    f"{tuple(src.shape)} {src.device}")
    C, H0, W0, ch = src.shape
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (C, H0, W0) or not mask.is_contiguous()
                             or mask.device != src.device):
        raise _lib.VolsurfsHipError(f"prepare_images: mask must be a contiguous uint8 [{C},{H0},{W0}] on {src.device}")
    s = int(subsample_factor)
    rgb = torch.empty(C, H0 // max(s, 1), W0 // max(s, 1), 3, device=src.device)
    out_mask = rgb.new_empty(rgb.shape[:3]) if (mask is not None or ch == 4) else None
    bg_host = (ctypes.c_float * 3)(*[float(v) for v in bg])
    _lib.call("vsa_images_prepare", src, mask, C, H0, W0, ch, s, ctypes.cast(bg_host, ctypes.c_void_p), rgb, out_mask,
              _lib.stream_ptr())
    return rgb, out_mask


# ---------------------------------------------------------------------------------------------------------- dataset

class DataCamera(Camera):
    """A `camera.Camera` of a loaded scene: every consumer of a Camera takes it unchanged.  `camera_idx` is the view's
    position in the scene's full list; `get_rgb()` / `get_mask()` are views of the split's device stacks."""

    def __init__(self, intrinsics, pose, height, width, camera_idx, device="cuda"):
        super().__init__(intrinsics, pose, height, width, device=device)
        self.camera_idx = int(camera_idx)
        self._pose = np.array(pose, np.float64).reshape(4, 4)
        self._intrinsics = np.array(intrinsics, np.float64).reshape(3, 3)
        self._stacks, self._slot = None, None

    def _attach(self, stacks, slot):
        self._stacks, self._slot = stacks, slot

    def get_pose(self):
        """Camera-to-world [4,4] f64 (x right, y down, z forward), as loaded and transformed."""
        return self._pose.copy()

    def get_intrinsics(self):
        """[3,3] f64, in pixels of the subsampled image."""
        return self._intrinsics.copy()

    def has_rgbs(self):
        return self._stacks is not None and self._stacks[0] is not None

    def has_masks(self):
        return self._stacks is not None and self._stacks[1] is not None

    def get_rgb(self):
        """[H,W,3] f32: a view of `MVDataset.images(split)`."""
        if not self.has_rgbs():
            raise ValueError("this camera has no image (the dataset was loaded with load_images=False)")
        return self._stacks[0][self._slot]

    def get_mask(self):
        """[H,W] f32: a view of `MVDataset.masks(split)`."""
        if not self.has_masks():
            raise ValueError("this camera has no mask")
        return self._stacks[1][self._slot]

    def get_opengl_projection_matrix(self, near=NEAR, far=FAR):
        return opengl_camera(self, near, far)[0]

    def get_opengl_matrix_world(self):
        return opengl_camera(self)[1]


class MVDataset:
    """A scene's cameras and images: `MVDataset(dataset_name, scene_name, datasets_path, splits, config, device)` reads
    `<datasets_path>/<dataset_name>/<scene_name>`.

    dataset_name: "blender", "blendernerf", "shelly" (`read_blender_split` per split) or "dtu" (`read_dtu_scene`; test =
    the views with index % test_camera_freq == 0, train = the others, or all of them with train_test_overlap).
    config: the parsed data config (see `DataParams`) or a DataParams.  The settings act on the fp64 poses before any
    Camera is made, in the order of `transform_poses`; then scene_radius = scene_radius_mult *
    (target_cameras_max_distance or 1), init_sphere_radius = scene_radius * init_sphere_scale; subsample_factor s divides
    fx, fy, cx, cy and gives H = H0 // s, W = W0 // s.  The Blender family's defaults (distance 1, multiplier 0.5) are
    chosen from nerf_synthetic's geometry and unverified against data.
    Images are decoded on the host (PIL, a thread pool), uploaded once as bytes and turned into `images(split)`
    [C,H,W,3] f32 and `masks(split)` [C,H,W] f32 by one `vsa_images_prepare` launch: composited over the background
    colour, subsampled, masks from `mask/` (DTU) or the alpha channel.  Only PNG is promised.  Everything that can be
    wrong with the files (a missing one, two sizes in a split) raises before anything is uploaded.
    load_images=False: cameras only (any device, "cpu" included)."""

    def __init__(self, dataset_name, scene_name, datasets_path, splits=("train", "test"), config=None, device="cuda",
                 load_images=True):
        if dataset_name not in DATASETS:
            raise ValueError(f"unknown dataset {dataset_name!r} (one of {', '.join(DATASETS)})")
        splits = list(splits)
        if not splits or len(set(splits)) != len(splits):
            raise ValueError(f"splits must name at least one split, each once, got {splits}")
        self.dataset_name, self.scene_name, self.device = dataset_name, scene_name, device
        self.params = config if isinstance(config, DataParams) else DataParams(dataset_name, scene_name, config)
        p = self.params
        self.bg_color = p.background()
        self.scene_dir = os.path.join(datasets_path, dataset_name, scene_name)
        if not os.path.isdir(self.scene_dir):
            raise FileNotFoundError(self.scene_dir)
        t0 = time.perf_counter()
        if dataset_name == "dtu":
            everything = read_dtu_scene(self.scene_dir)
            n = len(everything["index"])
            test = [i for i in range(n) if i % p.test_camera_freq == 0]
            keep = {"test": test, "train": list(range(n)) if p.train_test_overlap else
                    [i for i in range(n) if i % p.test_camera_freq != 0]}
            if any(s not in keep for s in splits):
                raise ValueError(f"a DTU scene has the splits train and test, got {splits}")
            recs = {s: _take(everything, keep[s]) for s in splits}
        else:
            recs = {s: read_blender_split(self.scene_dir, s, p.test_skip) for s in splits}
        if not p.load_mask:
            for rec in recs.values():
                rec["mask_paths"] = None
        poses, self.scene_scale = transform_poses({s: r["c2w"] for s, r in recs.items()}, p)
        self.scene_type = p.scene_type
        self.scene_radius = p.scene_radius_mult * (p.target_cameras_max_distance or 1.0)
        self.init_sphere_radius = self.scene_radius * p.init_sphere_scale
        s = p.subsample_factor
        # every file is decoded and checked before anything is uploaded
        t1 = time.perf_counter()
        raw = {name: self._decode(rec) for name, rec in recs.items()} if load_images else {}
        t2 = time.perf_counter()
        self.mv, self._stacks = {}, {}
        for name, rec in recs.items():
            H, W = rec["height"] // s, rec["width"] // s
            if H < 1 or W < 1:
                raise ValueError(f"subsample_factor {s} leaves nothing of a {rec['height']} x {rec['width']} image")
            stacks = self._prepare(*raw[name]) if load_images else (None, None)
            cams = []
            for slot, idx in enumerate(rec["index"]):
                K = rec["intrinsics"][slot].copy()
                K[:2] /= s
                cam = DataCamera(K, poses[name][slot], H, W, idx, device=device)
                if load_images:
                    cam._attach(stacks, slot)
                cams.append(cam)
            self.mv[name], self._stacks[name] = cams, stacks
        first = self.mv[splits[0]][0]
        self._height, self._width = first.height, first.width
        # host seconds: reading the cameras, decoding the files, and everything after (upload, launch, Cameras; the
        # device is not waited for)
        self.timings = {"parse_s": t1 - t0, "decode_s": t2 - t1, "prepare_s": time.perf_counter() - t2}

    def _decode(self, rec):
        src = _decode_stack(rec["image_paths"], _decode, "images")
        mask = None
        if rec["mask_paths"] is not None:
            mask = _decode_stack(rec["mask_paths"], _decode_mask, "masks")
            if mask.shape[:3] != src.shape[:3]:
                raise ValueError(f"masks are {mask.shape[1:3]}, images {src.shape[1:3]}")
        if (src.shape[1], src.shape[2]) != (rec["height"], rec["width"]):
            raise ValueError(f"images are {src.shape[1:3]}, the first header said {(rec['height'], rec['width'])}")
        return src, mask

    def _prepare(self, src, mask):
        if torch.device(self.device).type != "cuda":
            raise _lib.VolsurfsHipError("MVDataset: images are prepared on the GPU (device='cuda'); there is no CPU "
                                        "path.  load_images=False loads the cameras alone")
        src_d = torch.from_numpy(src).to(self.device)
        mask_d = None if mask is None else torch.from_numpy(mask).to(self.device)
        rgb, out_mask = prepare_images(src_d, mask_d, self.params.subsample_factor, self.bg_color)
        if not self.params.load_mask:
            out_mask = None
        return rgb, out_mask

    def __getitem__(self, split):
        return self.mv[split]

    def has_masks(self):
        return any(st[1] is not None for st in self._stacks.values())

    def get_width(self):
        return self._width

    def get_height(self):
        return self._height

    def images(self, split):
        """[C,H,W,3] f32 on the device."""
        rgb = self._stacks[split][0]
        if rgb is None:
            raise ValueError("the dataset was loaded with load_images=False")
        return rgb

    def masks(self, split):
        """[C,H,W] f32 on the device, or None."""
        return self._stacks[split][1]

    def splits(self, names=None):
        """{name: (cameras, images)}: the argument of `render_and_eval` and `EvalCallback`."""
        return {n: (self.mv[n], self.images(n)) for n in (names if names is not None else list(self.mv))}

    def reel(self, split="train"):
        """A `TensorReel` over the split, with its masks when present (the stacks are shared, not copied)."""
        return TensorReel(self.mv[split], self.images(split), self.masks(split), device=self.device)


def init_bounding_primitive(mv_data):
    """utils/volsurfs_utils.py:234-272: a box of side 2 scene_radius around a bounded scene, a sphere of radius 0.5
    around the foreground of an unbounded one."""
    if mv_data.scene_type == "bounded":
        return BoundingBox(side=2.0 * mv_data.scene_radius)
    if mv_data.scene_type == "unbounded":
        return BoundingSphere(0.5)
    raise ValueError(f"unknown scene type {mv_data.scene_type!r}: 'bounded' or 'unbounded'")


# ---------------------------------------------------------------------------------------------------------- writers

def _u8_stack(images, ndim, what):
    a = images.detach().cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    if a.dtype != np.uint8 or a.ndim != ndim or (ndim == 4 and a.shape[-1] not in (1, 3, 4)):
        raise ValueError(f"{what}: expected uint8 {'[C,H,W,1 | 3 | 4]' if ndim == 4 else '[C,H,W]'}, got {a.dtype} "
                         f"{a.shape}")
    return a


def _camera_arrays(cam):
    K = cam.intrinsics.detach().cpu().double().numpy()
    c2w = np.eye(4)
    c2w[:3, :4] = cam.c2w.detach().cpu().double().numpy()
    return K, c2w


def _save_png(path, a):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(a[..., 0] if a.ndim == 3 and a.shape[-1] == 1 else a).save(path)


def write_blender_scene(scene_dir, splits, bg=None):
    """The inverse of `read_blender_split`: splits = {name: (cameras, images_u8 [C,H,W,4 | 3 | 1])} ->
    `<scene_dir>/transforms_<name>.json` and `<scene_dir>/<name>/r_<i>.png`.  camera_angle_x = 2 atan(0.5 W / fx);
    transform_matrix = c2w . diag(1, -1, -1, 1), each fp32 entry written as the shortest decimal of its double, so
    that reading it back gives the same fp32 bits.  The format holds one pinhole per split with a centred principal
    point: a camera with fx != fy, a skew or another principal point raises ValueError.
    bg: None writes the images as they are; a colour ("white", "black" or a triple) flattens RGBA images over it first
    (8-bit: round((c a + bg 255 (255 - a)) / 255)) and writes RGB."""
    os.makedirs(scene_dir, exist_ok=True)
    for name, (cameras, images) in splits.items():
        a = _u8_stack(images, 4, f"split {name!r}")
        if len(cameras) != a.shape[0] or not cameras:
            raise ValueError(f"split {name!r}: {len(cameras)} cameras but {a.shape[0]} images")
        H, W = a.shape[1:3]
        if bg is not None and a.shape[-1] == 4:
            colour = np.asarray(_bg_color_of(bg), np.float64) * 255.0
            alpha = a[..., 3:4].astype(np.float64)
            a = np.rint((a[..., :3] * alpha + colour * (255.0 - alpha)) / 255.0).astype(np.uint8)
        K0, _ = _camera_arrays(cameras[0])
        frames = []
        for i, cam in enumerate(cameras):
            K, c2w = _camera_arrays(cam)
            if (cam.height, cam.width) != (H, W):
                raise ValueError(f"split {name!r}: camera {i} is {cam.height} x {cam.width}, the images {H} x {W}")
            if not (np.array_equal(K, K0) and K[0, 0] == K[1, 1] and K[0, 1] == 0.0 and K[0, 2] == 0.5 * W
                    and K[1, 2] == 0.5 * H):
                raise ValueError(f"split {name!r}: camera {i}: the format holds one focal length per split and a "
                                 "centred principal point")
            frames.append({"file_path": f"./{name}/r_{i}", "transform_matrix": opengl_to_camera(c2w).tolist()})
            _save_png(os.path.join(scene_dir, name, f"r_{i}.png"), a[i])
        meta = {"camera_angle_x": 2.0 * math.atan(0.5 * W / float(K0[0, 0])), "frames": frames}
        with open(os.path.join(scene_dir, f"transforms_{name}.json"), "w") as f:
            json.dump(meta, f, indent=1)


def write_dtu_scene(scene_dir, cameras, images_u8, masks_u8=None):
    """The inverse of `read_dtu_scene`: `cameras_sphere.npz` with scale_mat_i = I and world_mat_i = K [R | -R c] padded
    to 4x4 (fp64), `image/%06d.png` and, with masks_u8 [C,H,W], `mask/%03d.png`.
    The format stores the product K R, from which only an orthonormal R can be factored back out, and the fp32
    rotation of a Camera is orthonormal to fp32 only: R is the nearest rotation to it in fp64 (the polar factor), which
    it rounds back to within a few fp32 ulps, while the centre and the intrinsics return exactly."""
    a = _u8_stack(images_u8, 4, "images_u8")
    if len(cameras) != a.shape[0] or not cameras:
        raise ValueError(f"{len(cameras)} cameras but {a.shape[0]} images")
    masks = None
    if masks_u8 is not None:
        masks = _u8_stack(masks_u8, 3, "masks_u8")
        if masks.shape != a.shape[:3]:
            raise ValueError(f"masks_u8 is {masks.shape}, the images {a.shape[:3]}")
    os.makedirs(scene_dir, exist_ok=True)
    mats = {}
    for i, cam in enumerate(cameras):
        K, c2w = _camera_arrays(cam)
        u, _, vt = np.linalg.svd(c2w[:3, :3].T)
        R = u @ vt
        world = np.eye(4)
        world[:3, :3], world[:3, 3] = K @ R, -(K @ R) @ c2w[:3, 3]
        mats[f"world_mat_{i}"], mats[f"scale_mat_{i}"] = world, np.eye(4)
        _save_png(os.path.join(scene_dir, "image", f"{i:06d}.png"), a[i])
        if masks is not None:
            _save_png(os.path.join(scene_dir, "mask", f"{i:03d}.png"), masks[i])
    np.savez(os.path.join(scene_dir, "cameras_sphere.npz"), **mats)


__all__ = ["BLENDER_FAMILY", "DATASETS", "opengl_to_camera", "read_blender_split", "decompose_projection",
           "read_dtu_scene", "DataParams", "transform_poses", "prepare_images", "DataCamera", "MVDataset",
           "init_bounding_primitive", "write_blender_scene", "write_dtu_scene"]
