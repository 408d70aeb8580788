"""Device ray-caster of the robot's kinematic skeleton (include/h12render.h, csrc/h12_render.hip): what
``env.render()`` and ``gym.wrappers.RecordVideo`` show.  The image is defined in DESIGN.md section 7i.

The picture is a skeleton of capsules and boxes derived from the model JSON (``default_primitives``), not the robot's
visual mesh; one env per view, neighbouring envs are not drawn.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

MAX_PRIMS = 64
NOVERLAY = 10
CAPSULE, BOX = 1, 2
ID_SKY, ID_GROUND = -1, -2
ORIGIN_TYPES = {"world": 0, "asset_root": 1}
MARCH_STEP, NBISECT, MAX_FAR = 0.05, 16, 200.0
CHECKER, CHECKER_FAR, SHADOW_EPS = 0.5, 10.0, 1e-3

# display constants of the default skeleton (radii in metres, linear RGB)
# thigh / shank capsules: the radius shrinks down the leg, so the end caps of two links that meet at a joint origin
# are nested spheres and never the same surface (a depth tie over a whole cap)
LINK_RADIUS = 0.05
LINK_TAPER = 0.01
HIP_BAR_RADIUS = 0.05
KNEE_RADIUS = 0.055       # the knee collision segment, drawn thicker than the shank it sits in
TRUNK_RADIUS = 0.09
TRUNK_TOP = 0.45          # trunk capsule: pelvis origin to this height on the pelvis z axis
MIN_LINK_LENGTH = 0.1     # leg links shorter than this (hip and ankle offsets) get no capsule
COL_LEFT = (0.80, 0.35, 0.20)
COL_RIGHT = (0.20, 0.45, 0.80)
COL_TRUNK = (0.75, 0.75, 0.78)
COL_FOOT = (0.15, 0.15, 0.15)
COL_KNEE = (0.90, 0.80, 0.25)

RENDER_SYMBOLS = ["h12render_layout", "h12render_table_bytes", "h12render_pack_table", "h12render_render",
                  "h12render_last_error"]


class Prim(C.Structure):
    """h12render_prim"""
    _fields_ = [("type", C.c_int32), ("body", C.c_int32), ("p0", C.c_float * 3), ("p1", C.c_float * 3),
                ("radius", C.c_float), ("rgb", C.c_float * 3)]


class Camera(C.Structure):
    """h12render_camera"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("origin_type", C.c_int32), ("eye", C.c_float * 3),
                ("lookat", C.c_float * 3), ("fovy", C.c_float), ("sun_dir", C.c_float * 3), ("far", C.c_float)]


class Frame(C.Structure):
    """h12render_frame"""
    _fields_ = [("fstate", C.c_void_p), ("istate", C.c_void_p), ("n_envs", C.c_int32), ("env_ids", C.c_void_p),
                ("env_ids_host", C.POINTER(C.c_int32)), ("n_views", C.c_int32), ("view_origins", C.c_void_p),
                ("heights", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("hscale", C.c_float),
                ("x0", C.c_float), ("y0", C.c_float), ("table", C.c_void_p), ("n_prims", C.c_int32),
                ("overlays", C.c_int32), ("cull", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("rgb", C.c_void_p), ("id", C.c_void_p), ("depth", C.c_void_p)]


@dataclass
class ViewerCfg:
    """IsaacLab's ViewerCfg field names (eye, lookat, resolution, origin_type, env_index) plus the ray-caster's own.
    Unlike IsaacLab's default (a world camera at (7.5, 7.5, 7.5)), the default follows env 0's base and frames one
    robot."""

    eye: tuple = (2.2, 1.6, 0.6)
    lookat: tuple = (0.0, 0.0, -0.25)
    resolution: tuple = (640, 360)       # (width, height)
    origin_type: str = "asset_root"      # "world" | "asset_root"
    env_index: int = 0
    fovy_deg: float = 45.0
    sun_dir: tuple = (0.35, -0.25, 0.9)  # towards the sun; normalised on use
    overlays: bool = True
    supersample: int = 1
    far: float = 50.0


_bound = None


def render_library():
    """libh12env.so with the h12render_* prototypes set.  A library without them is an error (no fallback)."""
    global _bound
    if _bound is not None:
        return _bound
    from ._abi import H12EnvError, H12Model, load_library

    lib = load_library()
    for s in RENDER_SYMBOLS:
        if not hasattr(lib, s):
            raise H12EnvError(f"libh12env.so lacks {s}; rebuild it (csrc/h12_render.hip)")
    szp = C.POINTER(C.c_size_t)
    lib.h12render_layout.argtypes = [C.c_int, C.c_int, C.c_int, szp, szp, szp, szp]
    lib.h12render_layout.restype = C.c_int
    lib.h12render_table_bytes.argtypes = [C.c_int]
    lib.h12render_table_bytes.restype = C.c_size_t
    lib.h12render_pack_table.argtypes = [C.POINTER(H12Model), C.POINTER(Prim), C.c_int, C.c_void_p]
    lib.h12render_pack_table.restype = C.c_int
    lib.h12render_render.argtypes = [C.POINTER(Frame), C.POINTER(Camera), C.c_void_p]
    lib.h12render_render.restype = C.c_int
    lib.h12render_last_error.argtypes = []
    lib.h12render_last_error.restype = C.c_char_p
    _bound = lib
    return lib


def _check(lib, rc: int, what: str):
    if rc != 0:
        from ._abi import H12EnvError

        msg = lib.h12render_last_error()
        raise H12EnvError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def layout(n_views: int, width: int, height: int) -> dict:
    """Bytes of the scratch area and of the three outputs for n_views views of width x height."""
    lib = render_library()
    v = [C.c_size_t() for _ in range(4)]
    _check(lib, lib.h12render_layout(n_views, width, height, *[C.byref(x) for x in v]), "h12render_layout")
    return dict(zip(("scratch", "rgb", "id", "depth"), (x.value for x in v)))


def default_primitives(model) -> list[dict]:
    """The default skeleton, from the model constants alone: rows of
    {type, body, p0, p1, radius, rgb} (body 0 = pelvis, 1..12 in body_names order)."""
    rows = []

    def cap(body, p0, p1, r, rgb):
        rows.append(dict(type=CAPSULE, body=body, p0=tuple(float(x) for x in p0), p1=tuple(float(x) for x in p1),
                         radius=float(r), rgb=rgb))

    def box(body, c, h, rgb):
        rows.append(dict(type=BOX, body=body, p0=tuple(float(x) for x in c), p1=tuple(float(x) for x in h),
                         radius=0.0, rgb=rgb))

    parent = list(model.parent)
    jp = [tuple(model.joint_pos[j]) for j in range(12)]
    # trunk, torso collision box and hip bar on the pelvis
    cap(0, (0, 0, 0), (0, 0, TRUNK_TOP), TRUNK_RADIUS, COL_TRUNK)
    box(0, tuple(model.torso_center), tuple(model.torso_half), COL_TRUNK)
    roots = [j for j in range(12) if parent[j] == -1]
    cap(0, jp[roots[0]], jp[roots[1]], HIP_BAR_RADIUS, COL_TRUNK)
    rods = np.array([[[model.foot_rods[r][e][a] for a in range(3)] for e in range(2)] for r in range(4)]).reshape(-1, 3)
    fr = float(model.foot_radius)
    lo, hi = rods.min(0) - fr, rods.max(0) + fr
    for leg, root in enumerate(roots):
        col = COL_LEFT if leg == 0 else COL_RIGHT
        sy = 1.0 if leg == 0 else -1.0  # the right foot's rods mirror the left foot's (y -> -y)
        chain = [root]
        while True:
            nxt = [j for j in range(12) if parent[j] == chain[-1]]
            if not nxt:
                break
            chain.append(nxt[0])
        drawn = 0
        for j, child in zip(chain[:-1], chain[1:]):  # link of joint j is body j + 1; its child's joint origin
            if math.sqrt(sum(x * x for x in jp[child])) >= MIN_LINK_LENGTH:
                cap(j + 1, (0, 0, 0), jp[child], LINK_RADIUS - LINK_TAPER * drawn, col)
                drawn += 1
        knee = chain[3] + 1
        cap(knee, tuple(model.knee_p0), tuple(model.knee_p1), KNEE_RADIUS, COL_KNEE)
        c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        box(chain[-1] + 1, (c[0], sy * c[1], c[2]), h, COL_FOOT)
    return rows


def prim_array(rows) -> C.Array:
    arr = (Prim * max(len(rows), 1))()
    for i, r in enumerate(rows):
        p = arr[i]
        p.type, p.body, p.radius = int(r["type"]), int(r["body"]), float(r["radius"])
        p.p0[:], p.p1[:], p.rgb[:] = [float(x) for x in r["p0"]], [float(x) for x in r["p1"]], [float(x) for x in r["rgb"]]
    return arr


def pack_table(model, rows) -> np.ndarray:
    """The packed table of ``rows`` (host bytes, to be copied to the device once)."""
    lib = render_library()
    nbytes = lib.h12render_table_bytes(len(rows))
    if nbytes == 0:
        _check(lib, -1, "h12render_table_bytes")
    buf = np.zeros(nbytes, dtype=np.uint8)
    _check(lib, lib.h12render_pack_table(C.byref(model), prim_array(rows), len(rows), buf.ctypes.data),
           "h12render_pack_table")
    return buf


def camera_struct(viewer: ViewerCfg, scale: int = 1) -> Camera:
    if viewer.origin_type not in ORIGIN_TYPES:
        raise ValueError(f"viewer.origin_type: {viewer.origin_type!r} (world | asset_root)")
    cam = Camera()
    cam.width, cam.height = int(viewer.resolution[0]) * scale, int(viewer.resolution[1]) * scale
    cam.origin_type = ORIGIN_TYPES[viewer.origin_type]
    cam.eye[:], cam.lookat[:] = [float(x) for x in viewer.eye], [float(x) for x in viewer.lookat]
    cam.fovy = math.radians(viewer.fovy_deg)
    s = np.asarray(viewer.sun_dir, dtype=np.float64)
    nrm = float(np.linalg.norm(s))
    if not (nrm > 0 and math.isfinite(nrm)):
        raise ValueError("viewer.sun_dir: zero or not finite")
    cam.sun_dir[:] = [float(x) for x in s / nrm]
    cam.far = float(viewer.far)
    return cam


class Renderer:
    """The two launches of h12render_render over an env's workspace.  Scratch and outputs are allocated once per
    view count and reused: a returned tensor is overwritten by the next render() with the same number of views."""

    def __init__(self, env, viewer: ViewerCfg | None = None, prims=None, cull: bool = True):
        import torch

        self._torch = torch
        self._lib = render_library()
        self.env = env
        self.viewer = viewer if viewer is not None else (getattr(env.cfg, "viewer", None) or ViewerCfg())
        self.device = env.device
        self.rows = list(prims) if prims is not None else default_primitives(env._model)
        self.cull = bool(cull)
        self._table = torch.from_numpy(pack_table(env._model, self.rows)).to(self.device)
        ss = int(self.viewer.supersample)
        if ss not in (1, 2):
            raise ValueError(f"viewer.supersample: {ss} (1 | 2)")
        self._ss = ss
        self._cam = camera_struct(self.viewer, ss)
        self.width, self.height = int(self.viewer.resolution[0]), int(self.viewer.resolution[1])
        self._bufs: dict = {}
        self._ids: dict = {}

    def _view_ids(self, env_ids):
        key = tuple(int(i) for i in env_ids)
        hit = self._ids.get(key)
        if hit is None:
            torch = self._torch
            host = (C.c_int32 * len(key))(*key)
            dev = torch.tensor(key, dtype=torch.int32, device=self.device)
            hit = self._ids[key] = (host, dev)
        return hit

    def _buffers(self, m: int):
        b = self._bufs.get(m)
        if b is None:
            torch = self._torch
            w, h = self._cam.width, self._cam.height
            lay = layout(m, w, h)
            b = self._bufs[m] = dict(
                scratch=torch.zeros((lay["scratch"] + 15) // 16 * 4, dtype=torch.int32, device=self.device),
                rgb=torch.zeros((m, h, w, 3), dtype=torch.uint8, device=self.device),
                id=torch.zeros((m, h, w), dtype=torch.int32, device=self.device),
                depth=torch.zeros((m, h, w), dtype=torch.float32, device=self.device),
                origins=torch.zeros((m, 3), dtype=torch.float32, device=self.device))
        return b

    def render(self, env_ids=None, ids: bool = False, depth: bool = False):
        """rgb uint8 (M, H, W, 3) of the views ``env_ids`` (default: viewer.env_index), and with ids / depth the int32
        primitive ids (M, H, W) and the float32 ray distances.  Device tensors; no host synchronisation."""
        torch = self._torch
        env = self.env
        if env_ids is None:
            env_ids = [self.viewer.env_index]
        if self._ss != 1 and (ids or depth):
            raise ValueError("ids / depth are not defined with supersample > 1")
        host, dev = self._view_ids(env_ids)
        m = len(host)
        b = self._buffers(m)
        fr = Frame()
        fr.fstate, fr.istate, fr.n_envs = env._fstate.data_ptr(), env._istate.data_ptr(), env.num_envs
        fr.env_ids, fr.env_ids_host, fr.n_views = dev.data_ptr(), host, m
        t = env.terrain
        if t is not None:
            fr.heights, fr.nx, fr.ny = env._t_heights.data_ptr(), t.shape[0], t.shape[1]
            fr.hscale, fr.x0, fr.y0 = t.hscale, t.x0, t.y0
        else:
            torch.index_select(env.scene.env_origins, 0, dev.long(), out=b["origins"])
            fr.view_origins = b["origins"].data_ptr()
        fr.table, fr.n_prims = self._table.data_ptr(), len(self.rows)
        fr.overlays, fr.cull = int(bool(self.viewer.overlays)), int(self.cull)
        fr.scratch, fr.scratch_bytes = b["scratch"].data_ptr(), b["scratch"].numel() * 4
        fr.rgb = b["rgb"].data_ptr()
        fr.id = b["id"].data_ptr() if ids else None
        fr.depth = b["depth"].data_ptr() if depth else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(self._lib, self._lib.h12render_render(C.byref(fr), C.byref(self._cam), C.c_void_p(stream)),
               "h12render_render")
        rgb = b["rgb"]
        if self._ss != 1:  # box filter of the s x s samples
            s = self._ss
            acc = rgb.view(m, self.height, s, self.width, s, 3).to(torch.float32).mean(dim=(2, 4))
            rgb = torch.floor(acc + 0.5).to(torch.uint8)
        out = (rgb,)
        if ids:
            out += (b["id"],)
        if depth:
            out += (b["depth"],)
        return out[0] if len(out) == 1 else out

    def mosaic(self, env_ids, cols: int):
        """One frame (rows * H, cols * W, 3) tiling the views of ``env_ids`` row by row (unused cells black)."""
        torch = self._torch
        rgb = self.render(env_ids)
        m, h, w, _ = rgb.shape
        cols = max(1, int(cols))
        rows = (m + cols - 1) // cols
        full = torch.zeros((rows * cols, h, w, 3), dtype=torch.uint8, device=rgb.device)
        full[:m] = rgb
        return full.view(rows, cols, h, w, 3).permute(0, 2, 1, 3, 4).reshape(rows * h, cols * w, 3)
