"""Python mirror of the reference's host API over libgsplat.so.

Names follow the reference (nshelton/gaussian_splat):
  InstancedSplatRenderer  src/instanced_splat_renderer.h:13-34
  PLYLoader.load          src/ply_loader.h:30-44
  TrackballCamera         src/trackball_camera.h:5-64
with the Metal command buffer / drawable replaced by a HIP stream and an HBM
framebuffer (a torch CUDA tensor of shape (H, W, 4), fp32 RGBA, y down).

Matrices are 4x4 numpy arrays in math convention (M[row, col]); they cross
the C-ABI column-major, exactly like simd_float4x4.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from ._lib import GsOptions, GsSceneSoa, GsStats, check, lib

POINT_FLOATS = 62  # sizeof(PointData) / 4, src/ply_loader.h:7-28
RECORD_DTYPE = np.dtype([("cx", "<f4"), ("cy", "<f4"), ("ax", "<f4"), ("ay", "<f4"), ("bx", "<f4"),
                         ("by", "<f4"), ("opacity", "<f4"), ("r", "<f4"), ("g", "<f4"), ("b", "<f4"),
                         ("rect_lo", "<u4"), ("rect_hi", "<u4")])
MODES = {"tile": 0, "live50": 1, "mlab": 2}
BINNING = {"default": 0, "depth_first": 1, "bin_first": 2}  # gs_binning
MAX_FEATURE_CHANNELS = 64  # GS_MAX_FEATURE_CHANNELS (gs_render_features)
MAX_ID_SLOTS = 4  # GS_MAX_ID_SLOTS (gs_render_ids)
ID_NONE = 0xFFFFFFFF  # GS_ID_NONE: an empty slot of gs_render_ids


def _mat16(m) -> C.Array:
    a = np.asarray(m, dtype=np.float32)
    if a.shape == (4, 4):
        a = a.T  # math convention -> column-major
    a = np.ascontiguousarray(a.reshape(16), dtype=np.float32)
    return (C.c_float * 16)(*a.tolist())


def _from16(buf) -> np.ndarray:
    return np.array(list(buf), dtype=np.float32).reshape(4, 4).T.copy()


@dataclass
class Options:
    mode: str = "tile"
    sh_degree: int = 0
    crop: bool = True
    crop_radius: float = 5.0
    stage_timing: int = 0  # 0 off, 1 every stage (adds event gaps), 2 preprocess + composite only
    cap: int = 0  # per-pixel fragment cap by arrival order (0 = none; 32 tile shader, 50 live shader)
    frames_in_flight: int = 1  # 2: projection/sort of a frame overlaps the previous frame's composite
    # bin-list build order: "default" (per frame from the previous frame's pair count at this
    # resolution; depth-first on the first frame), "depth_first", "bin_first"
    binning: str = "default"
    # per-bin depth cuts (gs_options.depth_split; tile/live50 rules, no cap): a frame's
    # bin lists hold the pairs in front of the depth at which the bin's tiles saturated two frames
    # back, and a quadrant those lists leave open finishes from its saved state with the rest of
    # its bin's pairs.  Single-GPU frames, row-scheme rank renders and contiguous band renders alike.
    # The same image bit for bit, fewer pairs sorted; True is the default (False: whole lists)
    depth_split: bool = True

    def to_c(self) -> GsOptions:
        o = GsOptions()
        lib().gs_default_options(C.byref(o))
        if self.mode not in MODES:
            raise ValueError(f"mode must be one of {list(MODES)}")
        o.mode = MODES[self.mode]
        o.sh_degree = int(self.sh_degree)
        o.crop = int(bool(self.crop))
        o.crop_radius = float(self.crop_radius)
        o.stage_timing = int(self.stage_timing)
        if int(self.cap) < 0:
            raise ValueError("cap must be >= 0")
        o.cap = int(self.cap)
        if int(self.frames_in_flight) not in (1, 2):
            raise ValueError("frames_in_flight must be 1 or 2")
        o.frames_in_flight = int(self.frames_in_flight)
        if self.binning not in BINNING:
            raise ValueError(f"binning must be one of {list(BINNING)}")
        o.binning = BINNING[self.binning]
        o.depth_split = 1 if self.depth_split else 0
        return o


@dataclass
class Scene:
    """Host SoA scene (float32): activated values, as PLYLoader produces them."""
    pos: np.ndarray       # (N, 3)
    rot: np.ndarray       # (N, 4) w x y z raw
    scale: np.ndarray     # (N, 3) exp(scale)
    opacity: np.ndarray   # (N,) sigmoid(opacity)
    color: np.ndarray     # (N, 3) rgb (sh_degree 0) or raw f_dc (sh_degree > 0)
    sh_rest: Optional[np.ndarray] = None  # (N, 45) PLY order

    def __post_init__(self):
        for f in ("pos", "rot", "scale", "opacity", "color", "sh_rest"):
            v = getattr(self, f)
            if v is not None:
                setattr(self, f, np.ascontiguousarray(v, dtype=np.float32))

    @property
    def n(self) -> int:
        return int(self.pos.shape[0])

    @staticmethod
    def from_points(points: np.ndarray) -> "Scene":
        p = np.asarray(points, dtype=np.float32).reshape(-1, POINT_FLOATS)
        return Scene(pos=p[:, 0:3], rot=p[:, 13:17], scale=p[:, 10:13], opacity=p[:, 9], color=p[:, 6:9],
                     sh_rest=p[:, 17:62])

    def subset(self, sl) -> "Scene":
        return Scene(self.pos[sl], self.rot[sl], self.scale[sl], self.opacity[sl], self.color[sl],
                     None if self.sh_rest is None else self.sh_rest[sl])

    def to_c(self) -> GsSceneSoa:
        s = GsSceneSoa()
        s.n = self.n
        s.pos = self.pos.ctypes.data
        s.rot = self.rot.ctypes.data
        s.scale = self.scale.ctypes.data
        s.opacity = self.opacity.ctypes.data
        s.color = self.color.ctypes.data
        s.sh_rest = self.sh_rest.ctypes.data if self.sh_rest is not None else None
        return s


class PLYLoader:
    """src/ply_loader.h:30-44 — load() returns (ok, points[N, 62])."""

    @staticmethod
    def load(filepath: str, compat: bool = True) -> tuple[bool, np.ndarray]:
        ptr = L._FP()
        n = C.c_int64(0)
        st = lib().gs_ply_load(str(filepath).encode(), int(compat), C.byref(ptr), C.byref(n))
        pts = np.zeros((0, POINT_FLOATS), np.float32)
        if n.value > 0:
            pts = np.ctypeslib.as_array(ptr, shape=(n.value * POINT_FLOATS,)).reshape(-1, POINT_FLOATS).copy()
            lib().gs_ply_free(ptr)
        return st == 0, pts


def look_at(eye, center, up) -> np.ndarray:
    out = (C.c_float * 16)()
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    lib().gs_look_at(f3(eye), f3(center), f3(up), out)
    return _from16(out)


def perspective(fov_degrees: float, aspect: float, znear: float, zfar: float) -> np.ndarray:
    out = (C.c_float * 16)()
    lib().gs_perspective(float(fov_degrees), float(aspect), float(znear), float(zfar), out)
    return _from16(out)


class TrackballCamera:
    """src/trackball_camera.h:5-64 (matrix producers; defaults .mm:5-17, .h:28-37)."""

    def __init__(self):
        self.position = np.array([0.0, 0.0, 5.0], np.float32)
        self.target = np.zeros(3, np.float32)
        self.up = np.array([0.0, -1.0, 0.0], np.float32)
        self.distance = 5.0
        self.viewport = (800, 600)
        self.fov, self.nearPlane, self.farPlane = 45.0, 0.1, 1000.0
        self.minDistance, self.maxDistance = 0.1, 100.0

    def setViewportSize(self, w: int, h: int):
        self.viewport = (int(w), int(h))

    def setTarget(self, t):
        self.target = np.asarray(t, np.float32)

    def setPosition(self, p):
        self.position = np.asarray(p, np.float32)
        self.distance = float(np.linalg.norm(self.position - self.target))

    def setDistance(self, d: float):
        self.distance = min(max(d, self.minDistance), self.maxDistance)
        v = self.position - self.target
        self.position = self.target + v / np.linalg.norm(v) * self.distance

    def orbit(self, yaw: float, pitch: float = 0.0):
        """Rotate the eye about the target (trackball drag, .mm:55-83)."""
        off = self.position - self.target
        cy, sy = math.cos(yaw), math.sin(yaw)
        off = np.array([cy * off[0] + sy * off[2], off[1], -sy * off[0] + cy * off[2]], np.float32)
        if pitch:
            r = np.cross(-off, [0, 1, 0])
            r = r / np.linalg.norm(r)
            c, s = math.cos(pitch), math.sin(pitch)
            off = (off * c + np.cross(r, off) * s + r * np.dot(r, off) * (1 - c)).astype(np.float32)
        self.position = self.target + off

    def getViewMatrix(self) -> np.ndarray:
        return look_at(self.position, self.target, self.up)

    def getProjectionMatrix(self) -> np.ndarray:
        w, h = self.viewport
        return perspective(self.fov, np.float32(w) / np.float32(h), self.nearPlane, self.farPlane)


def default_camera(width: int, height: int) -> TrackballCamera:
    """The reference app's camera: eye (0,2,5), target 0 (src/main.mm:55-58)."""
    cam = TrackballCamera()
    cam.setViewportSize(width, height)
    cam.setPosition([0.0, 2.0, 5.0])
    cam.setTarget([0.0, 0.0, 0.0])
    return cam


class InstancedSplatRenderer:
    """src/instanced_splat_renderer.h:13-34 over libgsplat.so."""

    def __init__(self, source, options: Optional[Options] = None):
        self.options = options or Options()
        self._h = C.c_void_p()
        opt = self.options.to_c()
        if isinstance(source, Scene):
            self._scene_c = source.to_c()
            self._keep = source
            check(lib().gs_create_from_soa(C.byref(self._scene_c), C.byref(opt), C.byref(self._h)), "gs_create_from_soa")
        elif isinstance(source, np.ndarray):
            pts = np.ascontiguousarray(source, np.float32).reshape(-1, POINT_FLOATS)
            check(lib().gs_create_from_points(pts.ctypes.data, pts.shape[0], C.byref(opt), C.byref(self._h)),
                  "gs_create_from_points")
        else:
            check(lib().gs_create(str(source).encode(), C.byref(opt), C.byref(self._h)), "gs_create")
        self.device = None

    def initialize(self, device: int = 0) -> bool:
        check(lib().gs_initialize(self._h, int(device)), "gs_initialize")
        self.device = int(device)
        return True

    def getPointCount(self) -> int:
        return int(lib().gs_point_count(self._h))

    get_point_count = getPointCount

    def set_mode(self, mode: str):
        check(lib().gs_set_mode(self._h, MODES[mode]), "gs_set_mode")
        self.options.mode = mode

    def set_stage_timing(self, mode: int):
        """0 off, 1 every stage, 2 preprocess + composite via their own dispatch packets."""
        check(lib().gs_set_stage_timing(self._h, int(mode)), "gs_set_stage_timing")
        self.options.stage_timing = int(mode)

    def set_frames_in_flight(self, n: int):
        """1: every stage on the caller's stream; 2: a frame's projection/sort
        overlaps the previous frame's composite (internal stream)."""
        check(lib().gs_set_frames_in_flight(self._h, int(n)), "gs_set_frames_in_flight")
        self.options.frames_in_flight = int(n)

    def set_cap(self, cap: int):
        """Per-pixel fragment cap by arrival order (0 = none)."""
        check(lib().gs_set_cap(self._h, int(cap)), "gs_set_cap")
        self.options.cap = int(cap)

    def set_depth_split(self, on: bool):
        """Per-bin depth cuts (gs_set_depth_split): bin lists cut behind the depth
        where each bin saturated two frames back, open tiles finished by fallback
        lists; same image, bit for bit, less sorting."""
        check(lib().gs_set_depth_split(self._h, 1 if on else 0), "gs_set_depth_split")
        self.options.depth_split = bool(on)

    def render(self, view, proj, width: int, height: int, out=None, stream=None):
        """Render into `out` (torch float32 CUDA tensor (H, W, 4)); returns it."""
        import torch

        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=f"cuda:{self.device or 0}")
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == width * height * 4
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib().gs_render(self._h, _mat16(view), _mat16(proj), int(width), int(height), C.c_void_p(out.data_ptr()),
                              1, C.c_void_p(stream)), "gs_render")
        return out

    def render_depth(self, view, proj, width: int, height: int, out=None, depth=None, stream=None):
        """Render colour and depth in one composite pass (gs_render_depth): returns
        (rgba, depth), torch float32 CUDA tensors (H, W, 4) and (H, W).  `rgba` is
        render()'s frame bit for bit; `depth` is the accumulated view depth D
        (each splat's zF composited as a colour channel, 0 where nothing lands):
        in tile mode the expected depth is depth / rgba[..., 3] where alpha > 0.
        Tile and live50 modes without a fragment cap."""
        import torch

        dev = f"cuda:{self.device or 0}"
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=dev)
        if depth is None:
            depth = torch.empty((height, width), dtype=torch.float32, device=dev)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == width * height * 4
        assert depth.is_cuda and depth.dtype == torch.float32 and depth.is_contiguous() and depth.numel() == width * height
        assert depth.device == out.device
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib().gs_render_depth(self._h, _mat16(view), _mat16(proj), int(width), int(height),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(depth.data_ptr()), 1, C.c_void_p(stream)),
              "gs_render_depth")
        return out, depth

    def render_depth_host(self, view, proj, width: int, height: int):
        """render_depth into host memory: (rgba (H, W, 4), depth (H, W)) numpy float32."""
        out = np.empty((height, width, 4), np.float32)
        depth = np.empty((height, width), np.float32)
        check(lib().gs_render_depth(self._h, _mat16(view), _mat16(proj), int(width), int(height), out.ctypes.data,
                                    depth.ctypes.data, 0, None), "gs_render_depth")
        return out, depth

    def _feature_shape(self, features):
        """(N, K) of a feature matrix for this handle, or ValueError."""
        if getattr(features, "ndim", None) != 2:
            raise ValueError("features must be 2-D (N, K), one row per splat")
        n, k = int(features.shape[0]), int(features.shape[1])
        if n != self.getPointCount():
            raise ValueError(f"features has {n} rows, the scene has {self.getPointCount()} splats")
        if not 1 <= k <= MAX_FEATURE_CHANNELS:
            raise ValueError(f"features has {k} channels, 1..{MAX_FEATURE_CHANNELS} are supported")
        return n, k

    def render_features(self, view, proj, width: int, height: int, features, out=None, out_features=None,
                        stream=None):
        """Render colour and K per-splat feature channels composited per pixel
        (gs_render_features): returns (rgba, feats), torch float32 CUDA tensors
        (H, W, 4) and (H, W, K).  `features` is a torch float32 CUDA tensor (N, K),
        contiguous, row i for splat i of the loaded scene (get_scene's order);
        feats[y, x, k] is features[:, k] composited exactly as a colour channel
        (same fragments, order, weights and break rule; 0 where nothing lands; not
        clamped, not normalised).  `rgba` is render()'s frame bit for bit.  Tile and
        live50 modes without a fragment cap; the frame builds whole bin lists
        whatever depth_split says."""
        import torch

        if not isinstance(features, torch.Tensor):
            raise ValueError("features must be a torch tensor")
        n, k = self._feature_shape(features)
        if features.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {features.dtype}")
        if not features.is_contiguous():
            raise ValueError("features must be contiguous")
        dev = torch.device(f"cuda:{self.device or 0}")
        if not features.is_cuda or features.device != dev:
            raise ValueError(f"features must be on the handle's device {dev}, got {features.device}")
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=dev)
        if out_features is None:
            out_features = torch.empty((height, width, k), dtype=torch.float32, device=dev)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == width * height * 4
        assert (out_features.is_cuda and out_features.dtype == torch.float32 and out_features.is_contiguous()
                and out_features.numel() == width * height * k)
        assert out.device == dev and out_features.device == dev
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib().gs_render_features(self._h, _mat16(view), _mat16(proj), int(width), int(height),
                                       C.c_void_p(features.data_ptr() if n else None), k, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(out_features.data_ptr()), 1, C.c_void_p(stream)),
              "gs_render_features")
        return out, out_features

    def render_features_host(self, view, proj, width: int, height: int, features):
        """render_features from and into host memory: `features` a numpy float32
        array (N, K), C-contiguous; returns (rgba (H, W, 4), feats (H, W, K)) numpy float32."""
        if not isinstance(features, np.ndarray):
            raise ValueError("features must be a numpy array")
        n, k = self._feature_shape(features)
        if features.dtype != np.float32:
            raise ValueError(f"features must be float32, got {features.dtype}")
        if not features.flags["C_CONTIGUOUS"]:
            raise ValueError("features must be C-contiguous")
        out = np.empty((height, width, 4), np.float32)
        feats = np.empty((height, width, k), np.float32)
        check(lib().gs_render_features(self._h, _mat16(view), _mat16(proj), int(width), int(height),
                                       features.ctypes.data if n else None, k, out.ctypes.data, feats.ctypes.data, 0,
                                       None), "gs_render_features")
        return out, feats

    def render_contrib(self, view, proj, width: int, height: int, mask=None, out=None, sum=None, count=None,
                       max=None, accumulate: bool = False, stream=None):
        """Render colour and each splat's blend weight totals over the frame
        (gs_render_contrib): returns (rgba, sum, count, max).  For splat i of the
        loaded scene (get_scene's order) and every pixel the splat is composited at,
        the weight that multiplies its colour there is quantised to q = 0 .. 2**24;
        sum[i] is the total of q (torch.int64; sum / 2**24 is the splat's weight in
        pixels), count[i] the pixels with q > 0 and max[i] the largest q (torch.int32,
        holding the uint32 bits), CUDA tensors of N entries.  `mask`: a torch.uint8 or
        torch.bool (H, W) contiguous CUDA tensor of the pixels that count (None: all).
        accumulate=True combines the frame's totals into the three given tensors
        (sum +=, count +=, max = max) instead of overwriting them.  `rgba` is
        render()'s frame bit for bit.  Tile and live50 modes without a fragment cap;
        the frame builds whole bin lists whatever depth_split says."""
        import torch

        n = self.getPointCount()
        dev = torch.device(f"cuda:{self.device or 0}")
        if accumulate and (sum is None or count is None or max is None):
            raise ValueError("accumulate=True needs the sum, count and max tensors to combine into")

        def arr(t, name, dtype):
            if t is None:  # (allocated once every argument is judged)
                return None
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor")
            if t.dtype != dtype:
                raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
            if tuple(t.shape) != (n,):
                raise ValueError(f"{name} must have shape ({n},), got {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if not t.is_cuda or t.device != dev:
                raise ValueError(f"{name} must be on the handle's device {dev}, got {t.device}")
            return t

        if mask is not None:
            if not isinstance(mask, torch.Tensor):
                raise ValueError("mask must be a torch tensor")
            if mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError(f"mask must be uint8 or bool, got {mask.dtype}")
            if tuple(mask.shape) != (height, width):
                raise ValueError(f"mask must have shape ({height}, {width}), got {tuple(mask.shape)}")
            if not mask.is_contiguous():
                raise ValueError("mask must be contiguous")
            if not mask.is_cuda or mask.device != dev:
                raise ValueError(f"mask must be on the handle's device {dev}, got {mask.device}")
        sum = arr(sum, "sum", torch.int64)
        count = arr(count, "count", torch.int32)
        max = arr(max, "max", torch.int32)
        if sum is None:
            sum = torch.empty((n,), dtype=torch.int64, device=dev)
        if count is None:
            count = torch.empty((n,), dtype=torch.int32, device=dev)
        if max is None:
            max = torch.empty((n,), dtype=torch.int32, device=dev)
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=dev)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == width * height * 4
        assert out.device == dev
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib().gs_render_contrib(self._h, _mat16(view), _mat16(proj), int(width), int(height),
                                      C.c_void_p(mask.data_ptr() if mask is not None else None),
                                      C.c_void_p(out.data_ptr()), C.c_void_p(sum.data_ptr() if n else None),
                                      C.c_void_p(count.data_ptr() if n else None),
                                      C.c_void_p(max.data_ptr() if n else None), 1 if accumulate else 0, 1,
                                      C.c_void_p(stream)), "gs_render_contrib")
        return out, sum, count, max

    def render_contrib_host(self, view, proj, width: int, height: int, mask=None, sum=None, count=None, max=None,
                            accumulate: bool = False):
        """render_contrib from and into host memory: `mask` a numpy uint8 / bool array
        (H, W), C-contiguous, or None; returns (rgba (H, W, 4) float32, sum uint64,
        count uint32, max uint32) numpy arrays; accumulate=True combines into the three
        given arrays."""
        n = self.getPointCount()
        if accumulate and (sum is None or count is None or max is None):
            raise ValueError("accumulate=True needs the sum, count and max arrays to combine into")

        def arr(a, name, dtype):
            if a is None:
                return np.empty((n,), dtype)
            if not isinstance(a, np.ndarray):
                raise ValueError(f"{name} must be a numpy array")
            if a.dtype != dtype:
                raise ValueError(f"{name} must be {np.dtype(dtype)}, got {a.dtype}")
            if a.shape != (n,):
                raise ValueError(f"{name} must have shape ({n},), got {a.shape}")
            if not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
                raise ValueError(f"{name} must be C-contiguous and writeable")
            return a

        if mask is not None:
            if not isinstance(mask, np.ndarray):
                raise ValueError("mask must be a numpy array")
            if mask.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
                raise ValueError(f"mask must be uint8 or bool, got {mask.dtype}")
            if mask.shape != (height, width):
                raise ValueError(f"mask must have shape ({height}, {width}), got {mask.shape}")
            if not mask.flags["C_CONTIGUOUS"]:
                raise ValueError("mask must be C-contiguous")
        sum = arr(sum, "sum", np.uint64)
        count = arr(count, "count", np.uint32)
        max = arr(max, "max", np.uint32)
        out = np.empty((height, width, 4), np.float32)
        check(lib().gs_render_contrib(self._h, _mat16(view), _mat16(proj), int(width), int(height),
                                      mask.ctypes.data if mask is not None else None, out.ctypes.data,
                                      sum.ctypes.data if n else None, count.ctypes.data if n else None,
                                      max.ctypes.data if n else None, 1 if accumulate else 0, 0, None),
              "gs_render_contrib")
        return out, sum, count, max

    def render_ids(self, view, proj, width: int, height: int, slots: int = 4, out=None, ids=None, q=None, count=None,
                   want_q: bool = True, want_count: bool = True, stream=None):
        """Render colour and each pixel's top `slots` splats by blend weight
        (gs_render_ids): returns (rgba, ids, q, count), CUDA tensors (H, W, 4)
        float32 and (H, W, slots), (H, W, slots), (H, W) torch.int32 holding the
        uint32 bits.  The candidates of a pixel are the fragments the frame
        composites there with q > 0, q = 0 .. 2**24 being render_contrib's quantised
        weight; they are ordered by q descending, then splat index ascending.
        ids[y, x, k] is the k-th candidate's index into the loaded scene
        (get_scene's order), q[y, x, k] its weight, count[y, x] the number of
        candidates (it may exceed slots).  Empty slots hold ID_NONE (-1 as int32)
        and q = 0; every element is written, also where nothing lands.
        want_q=False / want_count=False leave that output out (None is returned in
        its place).  `rgba` is render()'s frame bit for bit.  Tile and live50 modes
        without a fragment cap; the frame builds whole bin lists whatever
        depth_split says."""
        import torch

        slots = int(slots)
        if not 1 <= slots <= MAX_ID_SLOTS:
            raise ValueError(f"slots must be 1..{MAX_ID_SLOTS}, got {slots}")
        dev = torch.device(f"cuda:{self.device or 0}")

        def arr(t, name, numel):
            if t is None:  # (allocated once every argument is judged)
                return None
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor")
            if t.dtype != torch.int32:
                raise ValueError(f"{name} must be torch.int32, got {t.dtype}")
            if t.numel() != numel:
                raise ValueError(f"{name} must have {numel} elements, got {t.numel()}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if not t.is_cuda or t.device != dev:
                raise ValueError(f"{name} must be on the handle's device {dev}, got {t.device}")
            return t

        px = int(width) * int(height)
        ids = arr(ids, "ids", px * slots)
        q = arr(q, "q", px * slots)
        count = arr(count, "count", px)
        if ids is None:
            ids = torch.empty((height, width, slots), dtype=torch.int32, device=dev)
        if q is None and want_q:
            q = torch.empty((height, width, slots), dtype=torch.int32, device=dev)
        if count is None and want_count:
            count = torch.empty((height, width), dtype=torch.int32, device=dev)
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=dev)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == px * 4
        assert out.device == dev
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib().gs_render_ids(self._h, _mat16(view), _mat16(proj), int(width), int(height), slots,
                                  C.c_void_p(out.data_ptr()), C.c_void_p(ids.data_ptr()),
                                  C.c_void_p(q.data_ptr() if q is not None else None),
                                  C.c_void_p(count.data_ptr() if count is not None else None), 1, C.c_void_p(stream)),
              "gs_render_ids")
        return out, ids, q, count

    def render_ids_host(self, view, proj, width: int, height: int, slots: int = 4, want_q: bool = True,
                        want_count: bool = True):
        """render_ids into host memory: (rgba (H, W, 4) float32, ids (H, W, slots),
        q (H, W, slots), count (H, W)) numpy arrays, the last three uint32 (None where
        not wanted)."""
        slots = int(slots)
        if not 1 <= slots <= MAX_ID_SLOTS:
            raise ValueError(f"slots must be 1..{MAX_ID_SLOTS}, got {slots}")
        out = np.empty((height, width, 4), np.float32)
        ids = np.empty((height, width, slots), np.uint32)
        q = np.empty((height, width, slots), np.uint32) if want_q else None
        count = np.empty((height, width), np.uint32) if want_count else None
        check(lib().gs_render_ids(self._h, _mat16(view), _mat16(proj), int(width), int(height), slots, out.ctypes.data,
                                  ids.ctypes.data, q.ctypes.data if want_q else None,
                                  count.ctypes.data if want_count else None, 0, None), "gs_render_ids")
        return out, ids, q, count

    def render_bgra8(self, view, proj, width: int, height: int, out=None, stream=None):
        """Render as BGRA8Unorm (the reference's drawable format) into `out`
        (torch uint8 CUDA tensor (H, W, 4), bytes B, G, R, A); returns it."""
        import torch

        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.uint8, device=f"cuda:{self.device or 0}")
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == width * height * 4
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib().gs_render_bgra8(self._h, _mat16(view), _mat16(proj), int(width), int(height),
                                    C.c_void_p(out.data_ptr()), 1, C.c_void_p(stream)), "gs_render_bgra8")
        return out

    def render_bgra8_host(self, view, proj, width: int, height: int) -> np.ndarray:
        out = np.empty((height, width, 4), np.uint8)
        check(lib().gs_render_bgra8(self._h, _mat16(view), _mat16(proj), int(width), int(height), out.ctypes.data,
                                    0, None), "gs_render_bgra8")
        return out

    def render_host(self, view, proj, width: int, height: int) -> np.ndarray:
        out = np.empty((height, width, 4), np.float32)
        check(lib().gs_render(self._h, _mat16(view), _mat16(proj), int(width), int(height), out.ctypes.data, 0, None),
              "gs_render")
        return out

    def last_stats(self) -> dict:
        s = GsStats()
        check(lib().gs_last_stats(self._h, C.byref(s)), "gs_last_stats")
        return s.as_dict()

    def kernel_times(self, max_frames: int = 64):
        """stage_timing 2: (ms_preprocess, ms_composite) arrays of the last
        frames (<= 64, oldest first) from the events in the kernels' dispatch packets."""
        pre = np.zeros(max_frames, np.float32)
        comp = np.zeros(max_frames, np.float32)
        cnt = C.c_int32(0)
        check(lib().gs_kernel_times(self._h, int(max_frames), pre.ctypes.data_as(C.POINTER(C.c_float)),
                                    comp.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cnt)), "gs_kernel_times")
        return pre[:cnt.value], comp[:cnt.value]

    def project_host(self, view, proj, width: int, height: int):
        n = self.getPointCount()
        rec = np.zeros(n, RECORD_DTYPE)
        dk = np.zeros(n, np.uint32)
        nt = np.zeros(n, np.uint32)
        check(lib().gs_project_host(self._h, _mat16(view), _mat16(proj), int(width), int(height), rec.ctypes.data,
                                    dk.ctypes.data, nt.ctypes.data), "gs_project_host")
        return rec, dk, nt

    def sorted_pairs(self):
        cnt = C.c_int64(0)
        check(lib().gs_sorted_pairs_host(self._h, None, None, 0, C.byref(cnt)), "gs_sorted_pairs_host")
        k = np.zeros(cnt.value, np.uint32)
        v = np.zeros(cnt.value, np.uint32)
        check(lib().gs_sorted_pairs_host(self._h, k.ctypes.data, v.ctypes.data, cnt.value, C.byref(cnt)),
              "gs_sorted_pairs_host")
        return k, v

    def scene(self) -> Scene:
        """The loaded (post-crop) scene as host SoA arrays (gs_get_scene)."""
        n = self.getPointCount()
        a = {k: np.empty(shape, np.float32) for k, shape in
             (("pos", (n, 3)), ("rot", (n, 4)), ("scale", (n, 3)), ("opacity", (n,)), ("color", (n, 3)),
              ("sh_rest", (n, 45)))}
        check(lib().gs_get_scene(self._h, *(a[k].ctypes.data for k in ("pos", "rot", "scale", "opacity", "color",
                                                                         "sh_rest"))), "gs_get_scene")
        return Scene(**a)

    def select(self, index):
        """Re-index the scene in place (gs_select): splat j of the new scene is
        splat index[j] of the old one.  Repeats are allowed and len(index) may
        exceed the old count; a permutation is the ordinary case; an empty
        index leaves an empty scene.  `index` is a 1-D CUDA tensor on the
        handle's device, torch.int32 (uint32 bit patterns, as render_ids returns
        them: ids[..., 0][mask] feeds straight in) or torch.int64 (range-checked
        and narrowed): the planes are gathered on the device; or a 1-D numpy
        integer array: the host path, which also works before initialize().
        The call waits for the frames in flight.  Afterwards every call sees the
        new scene, frames equal a fresh renderer's on scene().subset(index) bit
        for bit, and per-splat arguments and results are in the new order.  A
        rejected argument (an entry >= getPointCount()) leaves the scene as it
        was."""
        kind, a = self._splat_list(index, "index")
        if kind == "device":
            import torch

            stream = torch.cuda.current_stream(a.device).cuda_stream
            check(lib().gs_select(self._h, C.c_void_p(a.data_ptr() if a.numel() else None), int(a.numel()), 1,
                                  C.c_void_p(stream)), "gs_select")
        else:
            check(lib().gs_select(self._h, C.c_void_p(a.ctypes.data if a.size else None), int(a.size), 0, None),
                  "gs_select")

    def prune(self, keep):
        """Keep the splats with keep[i] != 0, in their order (gs_prune); returns
        the new -> old index map, whose length is the new count.  `keep` has
        getPointCount() entries: a 1-D CUDA tensor on the handle's device,
        torch.bool or torch.uint8 (the compaction and the gather run on the
        device; the map comes back as a torch.int32 CUDA tensor holding uint32
        bits), or a numpy bool / uint8 array (the host path, which also works
        before initialize(); the map is a numpy uint32 array).  The same as
        select(flatnonzero(keep))."""
        n = self.getPointCount()
        cnt = C.c_int64(0)
        try:
            import torch
        except ImportError:  # (numpy masks need no torch)
            torch = None
        if torch is not None and isinstance(keep, torch.Tensor):
            if keep.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"keep must be torch.bool or torch.uint8, got {keep.dtype}")
            dev = torch.device(f"cuda:{self.device or 0}")
            if not keep.is_cuda or keep.device != dev:
                raise ValueError(f"keep must be on the handle's device {dev}, got {keep.device}")
            if keep.dim() != 1 or keep.numel() != n:
                raise ValueError(f"keep must have {n} entries in one dimension, got shape {tuple(keep.shape)}")
            if not keep.is_contiguous():
                raise ValueError("keep must be contiguous")
            k8 = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
            if n == 0:  # (an empty tensor has no address to give)
                k8 = torch.zeros(1, dtype=torch.uint8, device=dev)
            out = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(lib().gs_prune(self._h, C.c_void_p(k8.data_ptr()), 1, C.c_void_p(out.data_ptr()), C.byref(cnt),
                                 C.c_void_p(stream)), "gs_prune")
            return out[:cnt.value]
        if not isinstance(keep, np.ndarray):
            raise ValueError("keep must be a torch CUDA tensor or a numpy array")
        if keep.dtype not in (np.dtype(np.bool_), np.dtype(np.uint8)):
            raise ValueError(f"keep must be bool or uint8, got {keep.dtype}")
        if keep.ndim != 1 or keep.size != n:
            raise ValueError(f"keep must have {n} entries in one dimension, got shape {keep.shape}")
        if not keep.flags.c_contiguous:
            raise ValueError("keep must be contiguous")
        k8 = keep.view(np.uint8) if n else np.zeros(1, np.uint8)
        out = np.empty(max(n, 1), np.uint32)
        check(lib().gs_prune(self._h, C.c_void_p(k8.ctypes.data), 0, C.c_void_p(out.ctypes.data), C.byref(cnt), None),
              "gs_prune")
        return out[:cnt.value].copy()

    def _splat_list(self, index, name):
        """An index list argument as ("device", int32 CUDA tensor) or ("host",
        uint32 numpy array); ValueError for anything else."""
        try:
            import torch
        except ImportError:  # (numpy lists need no torch)
            torch = None
        if torch is not None and isinstance(index, torch.Tensor):
            if index.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{name} must be torch.int32 or torch.int64, got {index.dtype}")
            dev = torch.device(f"cuda:{self.device or 0}")
            if not index.is_cuda or index.device != dev:
                raise ValueError(f"{name} must be on the handle's device {dev}, got {index.device}")
            if index.dim() != 1:
                raise ValueError(f"{name} must have one dimension, got shape {tuple(index.shape)}")
            if not index.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if index.numel() > 0xFFFFFFFE:
                raise ValueError(f"{name} holds more than 2**32 - 2 entries")
            if index.dtype == torch.int64:
                if index.numel() and (int(index.min()) < 0 or int(index.max()) > 0xFFFFFFFF):
                    raise ValueError(f"{name} entries must be 0 .. 2**32 - 1")
                index = index.to(torch.int32)  # (keeps the low 32 bits: the uint32 pattern)
            return "device", index
        if not isinstance(index, np.ndarray):
            raise ValueError(f"{name} must be a torch CUDA tensor or a numpy integer array")
        if index.dtype.kind not in "iu":
            raise ValueError(f"{name} must be an integer array, got {index.dtype}")
        if index.ndim != 1:
            raise ValueError(f"{name} must have one dimension, got shape {index.shape}")
        if not index.flags.c_contiguous:
            raise ValueError(f"{name} must be contiguous")
        if index.size > 0xFFFFFFFE:
            raise ValueError(f"{name} holds more than 2**32 - 2 entries")
        if index.dtype == np.int32:  # (uint32 bit patterns, as render_ids_host's ids viewed as int32)
            return "host", index.view(np.uint32)
        if index.dtype != np.uint32:
            if index.size and (int(index.min()) < 0 or int(index.max()) > 0xFFFFFFFF):
                raise ValueError(f"{name} entries must be 0 .. 2**32 - 1")
            index = index.astype(np.uint32)
        return "host", index

    def subset(self, begin: int, end: int) -> "InstancedSplatRenderer":
        """A renderer over splats [begin, end) of this one's scene (gs_create_subset)."""
        r = InstancedSplatRenderer.__new__(InstancedSplatRenderer)
        r.options = Options(**vars(self.options))
        r._h = C.c_void_p()
        r.device = None
        check(lib().gs_create_subset(self._h, int(begin), int(end), C.byref(r._h)), "gs_create_subset")
        return r

    def close(self):
        if self._h:
            lib().gs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def radix_sort_pairs(keys, vals, bits: int, stream=None):
    """Stable LSD sort of torch uint32-as-int32 CUDA tensors in place."""
    import torch

    n = keys.numel()
    tk = torch.empty_like(keys)
    tv = torch.empty_like(vals)
    if stream is None:
        stream = torch.cuda.current_stream(keys.device).cuda_stream
    check(lib().gs_radix_sort_pairs(C.c_void_p(keys.data_ptr()), C.c_void_p(vals.data_ptr()),
                                    C.c_void_p(tk.data_ptr()), C.c_void_p(tv.data_ptr()), n, int(bits),
                                    C.c_void_p(stream)), "gs_radix_sort_pairs")
    return keys, vals


SCHEMES = {"rows": 0, "slabs": 1, "bands": 2}  # gs_scheme
TRANSPORTS = {"auto": 0, "rccl": 1, "copy": 2}  # gs_transport


class ShardedGroup:
    """Multi-GPU frames from one process (gs_create_sharded):
    one contiguous splat-index shard per device, frames into devices[0] by
    the bin-row scheme (bit-identical to one GPU) or the depth-slab scheme;
    RCCL when every rank has its own device, peer copies otherwise."""

    def __init__(self, source, num_gpus: int, options: Optional[Options] = None, replicated: bool = False):
        """replicated: every rank holds the whole scene (gs_create_replicated),
        rendering its own bin rows ("bands")."""
        self.options = options or Options()
        self._g = C.c_void_p()
        kind = "replicated" if replicated else "sharded"
        if isinstance(source, InstancedSplatRenderer):
            check(getattr(lib(), f"gs_create_{kind}_from_handle")(source._h, int(num_gpus), C.byref(self._g)),
                  f"gs_create_{kind}_from_handle")
        else:
            opt = self.options.to_c()
            check(getattr(lib(), f"gs_create_{kind}")(str(source).encode(), C.byref(opt), int(num_gpus),
                                                       C.byref(self._g)), f"gs_create_{kind}")
        self.device = None

    def initialize(self, devices=None, transport: str = "auto") -> bool:
        arr = None
        if devices is not None:
            d = np.ascontiguousarray(devices, np.int32)
            assert d.shape == (self.size,)
            arr = d.ctypes.data
            self._devices = d
        check(lib().gs_group_initialize(self._g, arr, TRANSPORTS[transport]), "gs_group_initialize")
        self.device = int(devices[0]) if devices is not None else 0
        return True

    @property
    def size(self) -> int:
        return int(lib().gs_group_size(self._g))

    @property
    def transport(self) -> str:
        t = int(lib().gs_group_transport(self._g))
        return {v: k for k, v in TRANSPORTS.items()}.get(t, "none")

    def getPointCount(self) -> int:
        return int(lib().gs_group_point_count(self._g))

    def set_scheme(self, scheme: str):
        check(lib().gs_group_set_scheme(self._g, SCHEMES[scheme]), "gs_group_set_scheme")

    def set_timeout(self, timeout_ms: int):
        """Bound of every host wait (gs_group_set_timeout): an expired wait or
        an RCCL peer error aborts the communicators and raises (GS_ERR_COMM)."""
        check(lib().gs_group_set_timeout(self._g, int(timeout_ms)), "gs_group_set_timeout")

    def render(self, view, proj, width: int, height: int, out=None, stream=None):
        import torch

        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=f"cuda:{self.device or 0}")
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == width * height * 4
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib().gs_group_render(self._g, _mat16(view), _mat16(proj), int(width), int(height),
                                    C.c_void_p(out.data_ptr()), 1, C.c_void_p(stream)), "gs_group_render")
        return out

    def render_host(self, view, proj, width: int, height: int) -> np.ndarray:
        out = np.empty((height, width, 4), np.float32)
        check(lib().gs_group_render(self._g, _mat16(view), _mat16(proj), int(width), int(height), out.ctypes.data,
                                    0, None), "gs_group_render")
        return out

    def set_frames_in_flight(self, n: int):
        """2: rows frames pipelined (gs_group_render_pipelined), one frame's
        all-to-all under the previous frame's render and gather."""
        check(lib().gs_group_set_frames_in_flight(self._g, int(n)), "gs_group_set_frames_in_flight")

    def render_pipelined(self, view, proj, width: int, height: int, out=None, stream=None, host: bool = False):
        """Projects this view's frame and returns the PREVIOUS call's frame
        (None on the first call): a device tensor on the caller's stream, or
        with host=True a numpy array.  flush() returns the last one."""
        return self._pipelined(view, proj, width, height, out, stream, host)

    def flush(self, width: int = 0, height: int = 0, out=None, stream=None, host: bool = False):
        """The frame still in flight (None when there is none); its size is
        the one it was projected at."""
        return self._pipelined(None, None, width, height, out, stream, host)

    def _pipelined(self, view, proj, width, height, out, stream, host):
        import torch

        produced = C.c_int32(0)
        # (the frame that comes back is the one in flight: its size, not this view's)
        prev = getattr(self, "_inflight", None)
        self._inflight = (width, height) if view is not None else None
        ow, oh = prev if prev is not None else (width, height)
        if host:
            buf = np.empty((oh, ow, 4), np.float32)
            ptr, dev_out, st = buf.ctypes.data, 0, None
        else:
            if out is None:
                out = torch.empty((oh, ow, 4), dtype=torch.float32, device=f"cuda:{self.device or 0}")
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
            assert out.numel() >= ow * oh * 4, "out holds the frame in flight (the previous call's size)"
            buf, ptr, dev_out = out, out.data_ptr(), 1
            st = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
        if view is None:
            check(lib().gs_group_flush(self._g, C.c_void_p(ptr), dev_out, C.c_void_p(st), C.byref(produced)),
                  "gs_group_flush")
        else:
            check(lib().gs_group_render_pipelined(self._g, _mat16(view), _mat16(proj), int(width), int(height),
                                                  C.c_void_p(ptr), dev_out, C.c_void_p(st), C.byref(produced)),
                  "gs_group_render_pipelined")
        return buf if produced.value else None

    def last_stats(self, rank: int = 0) -> dict:
        s = GsStats()
        check(lib().gs_group_last_stats(self._g, int(rank), C.byref(s)), "gs_group_last_stats")
        return s.as_dict()

    def close(self):
        if self._g:
            lib().gs_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
