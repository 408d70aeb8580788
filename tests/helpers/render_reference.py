"""CPU reference of the ray-caster's image, restated in numpy from the definition; it shares
no code with csrc/h12_render.hip.  ``dtype`` switches every operation between float64 and float32: the float32 run
measures the definition's own rounding sensitivity (tests/golden/render_gates.json), the float64 run is the truth.

    render(scene_view, dtype) -> dict(rgb uint8 (H, W, 3), id int32 (H, W), depth (H, W), parity, lit)

A view is described by plain data (see ``View``): the env's state columns, the model dict, the primitive rows, the
camera, the env origin and optionally the heightfield."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

MARCH_STEP, NBISECT = 0.05, 16
CHECKER, CHECKER_FAR, SHADOW_EPS = 0.5, 10.0, 1e-3
AMBIENT, DIFFUSE = 0.35, 0.65
COL_CHK = ((0.55, 0.55, 0.55), (0.35, 0.35, 0.35))
COL_FAR = (0.45, 0.45, 0.45)
COL_HORIZON, COL_ZENITH = (0.80, 0.86, 0.93), (0.30, 0.50, 0.85)
CONTACT_RADIUS, COL_CONTACT = 0.02, (1.0, 0.15, 0.1)
ARROW_RADIUS, ARROW_GAIN, ARROW_Z, ARROW_DZ, ARROW_MIN = 0.012, 0.5, 0.55, 0.05, 1e-3
COL_CMD, COL_VEL = (0.1, 0.8, 0.2), (0.1, 0.3, 1.0)
CAPSULE, BOX = 1, 2
ID_SKY, ID_GROUND = -1, -2


@dataclass
class View:
    pos: np.ndarray            # (3,) workspace POS (env-local on the plane, world on a heightfield)
    quat: np.ndarray           # (4,) w x y z
    q: np.ndarray              # (12,)
    vlin: np.ndarray           # (3,)
    cmd: np.ndarray            # (2,)
    pack: int                  # H12_I_PACK word
    origin: np.ndarray         # (3,) env origin: view origin on the plane, H12_F_ORIGIN on a heightfield
    model: dict                # the model JSON
    rows: list                 # primitive rows {type, body, p0, p1, radius, rgb}
    width: int = 96
    height: int = 64
    eye: tuple = (2.0, 1.2, 0.4)
    lookat: tuple = (0.0, 0.0, -0.3)
    origin_type: str = "asset_root"
    fovy_deg: float = 45.0
    sun_dir: tuple = (0.35, -0.25, 0.9)
    far: float = 50.0
    overlays: bool = True
    terrain: object = None     # h12env.terrain.Terrain or None (plane)
    extra: dict = field(default_factory=dict)


def fk(model: dict, pos, quat, q, dtype=np.float64):
    """World rotation (13, 3, 3) and origin (13, 3) of every body: axis-aligned joints, pure-translation offsets."""
    T = dtype
    w, x, y, z = (T(v) for v in quat)
    n = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    R = np.zeros((13, 3, 3), dtype=T)
    p = np.zeros((13, 3), dtype=T)
    R[0] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=T)
    p[0] = np.asarray(pos, dtype=T)
    for j, jd in enumerate(model["joints"]):
        par = int(jd["parent"]) + 1
        a = T(q[j])
        c, s = np.cos(a), np.sin(a)
        Rj = np.eye(3, dtype=T)
        ax = int(jd["axis"])
        if ax == 0:
            Rj[1, 1], Rj[1, 2], Rj[2, 1], Rj[2, 2] = c, -s, s, c
        elif ax == 1:
            Rj[0, 0], Rj[0, 2], Rj[2, 0], Rj[2, 2] = c, s, -s, c
        else:
            Rj[0, 0], Rj[0, 1], Rj[1, 0], Rj[1, 1] = c, -s, s, c
        R[j + 1] = (R[par] @ Rj).astype(T)
        p[j + 1] = p[par] + R[par] @ np.asarray(jd["pos"], np.float32).astype(T)  # the model struct holds float32
    return R, p


def _dot(a, b):
    return (a * b).sum(-1)


def hit_capsule(o, v, a, d, r, T):
    """Entry distance (inf = none) and outward normal of rays (o, v) into the capsule (a, a + d, r)."""
    inf = T(np.inf)
    oa = o - a
    baba, bard, baoa, rdoa, oaoa = _dot(d, d), _dot(v, d), _dot(oa, d), _dot(v, oa), _dot(oa, oa)
    A = baba - bard * bard
    B = baba * rdoa - baoa * bard
    Cc = baba * oaoa - baoa * baoa - r * r * baba
    par = ~(A > T(1e-8) * baba)
    with np.errstate(all="ignore"):
        h = B * B - A * Cc
        miss_cyl = ~par & (h < 0)
        tb = (-B - np.sqrt(np.where(h < 0, 0, h))) / np.where(par, 1, A)
        y = np.where(par, np.where(bard > 0, T(-1), baba + 1), baoa + tb * bard)
        body = ~par & ~miss_cyl & (y > 0) & (y < baba)
        nb = (oa + tb[:, None] * v - d * (y / np.where(baba > 0, baba, 1))[:, None]) / r
        oc = np.where((y <= 0)[:, None], oa, oa - d)
        b2, c2 = _dot(v, oc), _dot(oc, oc) - r * r
        h2 = b2 * b2 - c2
        tc = -b2 - np.sqrt(np.where(h2 > 0, h2, 0))
        cap = ~body & ~miss_cyl & (h2 > 0)
        nc = (oc + tc[:, None] * v) / r
    t = np.where(body, tb, np.where(cap, tc, inf))
    t = np.where(t > 0, t, inf).astype(T)
    nrm = np.where(body[:, None], nb, nc).astype(T)
    return t, nrm


def hit_box(o, v, c, R, hh, T):
    inf = T(np.inf)
    ol = (o - c) @ R  # components along the box axes (columns of R)
    vl = v @ R
    n = o.shape[0]
    tn = np.full(n, -inf, dtype=T)
    tf = np.full(n, inf, dtype=T)
    axis = np.zeros(n, dtype=np.int64)
    sgn = np.zeros(n, dtype=T)
    miss = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            parl = np.abs(vl[:, i]) < T(1e-12)
            miss |= parl & (np.abs(ol[:, i]) > hh[i])
            inv = 1 / np.where(parl, 1, vl[:, i])
            t1, t2 = (-hh[i] - ol[:, i]) * inv, (hh[i] - ol[:, i]) * inv
            lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
            upd = ~parl & (lo > tn)
            tn = np.where(upd, lo, tn)
            axis = np.where(upd, i, axis)
            sgn = np.where(upd, np.where(vl[:, i] > 0, T(-1), T(1)), sgn)
            tf = np.where(parl, tf, np.minimum(tf, hi))
    ok = ~miss & (tn < tf) & (tn > 0)
    t = np.where(ok, tn, inf).astype(T)
    nrm = (sgn[:, None] * R.T[axis]).astype(T)
    return t, nrm


def ground_height(terrain, org, xl, yl, T):
    """Height relative to the env origin, and slopes, of the triangle mesh at env-local (xl, yl): cells split along
    the (ix, iy) -> (ix + 1, iy + 1) diagonal, flat border outside the grid."""
    nx, ny = terrain.heights.shape
    hs = T(terrain.hscale)
    u = np.clip((xl + org[0] - T(terrain.x0)) / hs, T(0), T(nx - 1) - T(1e-3))
    w = np.clip((yl + org[1] - T(terrain.y0)) / hs, T(0), T(ny - 1) - T(1e-3))
    ix, iy = u.astype(np.int64), w.astype(np.int64)
    fu, fv = u - ix.astype(T), w - iy.astype(T)
    H = terrain.heights.astype(T)
    h00, h01, h10, h11 = H[ix, iy], H[ix, iy + 1], H[ix + 1, iy], H[ix + 1, iy + 1]
    up = fv >= fu
    a = np.where(up, h11 - h01, h10 - h00)
    b = np.where(up, h01 - h00, h11 - h10)
    return (h00 + fu * a + fv * b - org[2]).astype(T), (a / hs).astype(T), (b / hs).astype(T)


def world_prims(view: View, R, p, valid: bool, T):
    """The table rows and the overlay rows in the view's env frame: list of (type, A, D, radius, rgb, axes) or None."""
    out = []
    if not valid:
        return out
    for r in view.rows:
        b = int(r["body"])
        p0, p1 = np.asarray(r["p0"], np.float32).astype(T), np.asarray(r["p1"], np.float32).astype(T)
        rgb = np.asarray(r["rgb"], np.float32).astype(T)
        a = p[b] + R[b] @ p0
        if int(r["type"]) == CAPSULE:
            out.append((CAPSULE, a, R[b] @ (p1 - p0), T(np.float32(r["radius"])), rgb, None))
        else:
            out.append((BOX, a, p1, T(0), rgb, R[b]))
    if view.overlays:
        pts = np.asarray(view.model["foot"]["points"], np.float32).astype(T)
        for o in range(8):
            if (int(view.pack) >> (13 + o)) & 1:
                b = 6 * (o // 4) + 6
                out.append((CAPSULE, p[b] + R[b] @ pts[o % 4], np.zeros(3, T), T(np.float32(CONTACT_RADIUS)),
                            np.asarray(COL_CONTACT, np.float32).astype(T), None))
            else:
                out.append(None)
        hx, hy = R[0][0, 0], R[0][1, 0]
        hn = np.sqrt(hx * hx + hy * hy)
        vb = R[0].T @ np.asarray(view.vlin, np.float32).astype(T)
        for o, (vx, vy) in ((8, (T(np.float32(view.cmd[0])), T(np.float32(view.cmd[1])))), (9, (vb[0], vb[1]))):
            sp = np.sqrt(vx * vx + vy * vy)
            if hn > T(1e-6) and sp > T(np.float32(ARROW_MIN)):
                ux, uy = hx / hn, hy / hn
                g = T(np.float32(ARROW_GAIN))
                a = p[0] + np.array([0, 0, T(np.float32(ARROW_Z)) + (T(np.float32(ARROW_DZ)) if o == 9 else T(0))], T)
                d = np.array([g * (vx * ux - vy * uy), g * (vx * uy + vy * ux), 0], T)
                out.append((CAPSULE, a, d, T(np.float32(ARROW_RADIUS)),
                            np.asarray(COL_CMD if o == 8 else COL_VEL, np.float32).astype(T), None))
            else:
                out.append(None)
    return out


def _hit(pr, o, v, T):
    kind, a, d, r, _, axes = pr
    return hit_capsule(o, v, a, d, r, T) if kind == CAPSULE else hit_box(o, v, a, axes, d, T)


def render(view: View, dtype=np.float64, shift=(0.0, 0.0)) -> dict:
    """The image of ``view``; ``shift`` moves every pixel centre by that many pixels (x, y)."""
    T = dtype
    W, Hh = view.width, view.height
    f32 = lambda x: np.asarray(x, np.float32).astype(T)  # noqa: E731  (inputs are float32 data)
    parts = [np.ravel(view.pos), np.ravel(view.quat), np.ravel(view.q)]
    if view.overlays:
        parts += [np.ravel(view.vlin), np.ravel(view.cmd)]
    state = np.concatenate(parts).astype(np.float64)
    org = f32(view.origin)
    valid = bool(np.isfinite(state).all() and np.isfinite(org).all())
    if valid:
        valid = float(np.sum(np.asarray(view.quat, np.float64) ** 2)) > 1e-30
    if not np.isfinite(org).all():
        org = np.zeros(3, T)
    if valid:
        pos = f32(view.pos) - org if view.terrain is not None else f32(view.pos)
        R, p = fk(view.model, pos, f32(view.quat), f32(view.q), T)
    else:  # background only; the base stands in at its initial height for an asset_root camera
        R, p = fk(view.model, np.array([0, 0, 1.05], np.float32).astype(T), np.array([1, 0, 0, 0], T), np.zeros(12, T), T)
    prims = world_prims(view, R, p, valid, T)
    eye_o, la_o = f32(view.eye), f32(view.lookat)
    base = p[0] if view.origin_type == "asset_root" else np.zeros(3, T)
    eye = base + eye_o
    fwd = la_o - eye_o
    fwd = fwd / np.sqrt(_dot(fwd, fwd))
    rgt = np.array([fwd[1], -fwd[0], 0], T)
    rgt = rgt / np.sqrt(_dot(rgt, rgt))
    up = np.cross(rgt, fwd).astype(T)
    th = T(np.float32(np.tan(0.5 * np.float64(np.float32(np.radians(view.fovy_deg))))))  # passed as float32
    jj, ii = np.meshgrid(np.arange(W), np.arange(Hh))
    x = (((jj.ravel().astype(T) + T(0.5) + T(shift[0])) / T(W)) * 2 - 1) * (th * T(W) / T(Hh))
    y = -((((ii.ravel().astype(T) + T(0.5) + T(shift[1])) / T(Hh)) * 2 - 1)) * th
    d = fwd[None, :] + x[:, None] * rgt[None, :] + y[:, None] * up[None, :]
    d = (d / np.sqrt(_dot(d, d))[:, None]).astype(T)
    N = d.shape[0]
    o = np.broadcast_to(eye, (N, 3)).astype(T)
    inf = T(np.inf)
    sun = f32(view.sun_dir)
    sun = sun / np.sqrt(_dot(sun, sun))
    sun = np.asarray(sun, np.float32).astype(T)  # the kernel receives the normalised vector as float32

    tbest = np.full(N, inf, T)
    best = np.full(N, ID_SKY, np.int64)
    nbest = np.zeros((N, 3), T)
    for k, pr in enumerate(prims):
        if pr is None:
            continue
        t, nrm = _hit(pr, o, d, T)
        upd = t < tbest
        tbest = np.where(upd, t, tbest)
        best = np.where(upd, k, best)
        nbest = np.where(upd[:, None], nrm, nbest)
    # ground
    tg = np.full(N, inf, T)
    ng = np.zeros((N, 3), T)
    ng[:, 2] = 1
    far = T(np.float32(view.far))
    if view.terrain is None:
        with np.errstate(all="ignore"):
            ok = (d[:, 2] < 0) & (eye[2] > 0)
            tg = np.where(ok, eye[2] / np.where(ok, -d[:, 2], 1), inf).astype(T)
    else:
        n_march = int(np.ceil(np.float64(np.float32(view.far)) / np.float64(np.float32(MARCH_STEP))))
        step = T(np.float32(MARCH_STEP))
        gfun = lambda t, m: o[m, 2] + t * d[m, 2] - ground_height(  # noqa: E731
            view.terrain, org, o[m, 0] + t * d[m, 0], o[m, 1] + t * d[m, 1], T)[0]
        live = np.ones(N, bool)
        lo = np.zeros(N, T)
        for k in range(1, n_march + 1):
            live &= ~(lo >= tbest)
            idx = np.nonzero(live)[0]
            if idx.size == 0:
                break
            hi = T(k) * step
            g = gfun(np.full(idx.size, hi, T), idx)
            hitm = idx[g <= 0]
            if hitm.size:
                a, b = lo[hitm].copy(), np.full(hitm.size, hi, T)
                for _ in range(NBISECT):
                    mid = T(0.5) * (a + b)
                    below = gfun(mid, hitm) <= 0
                    b = np.where(below, mid, b)
                    a = np.where(below, a, mid)
                tg[hitm] = b
                _, gx, gy = ground_height(view.terrain, org, o[hitm, 0] + b * d[hitm, 0], o[hitm, 1] + b * d[hitm, 1], T)
                inv = 1 / np.sqrt(gx * gx + gy * gy + 1)
                ng[hitm] = np.stack([-gx * inv, -gy * inv, inv], -1)
                live[hitm] = False
            lo[idx] = hi
    tg = np.where((tg > 0) & (tg < far), tg, inf).astype(T)
    gnd = tg < tbest
    hit = gnd | (best >= 0)
    th_ = np.where(gnd, tg, tbest)
    nh = np.where(gnd[:, None], ng, nbest)
    with np.errstate(all="ignore"):
        hp = o + np.where(hit, th_, 0)[:, None] * d
    # albedo
    alb = np.zeros((N, 3), T)
    parity = np.full(N, -1, np.int64)
    wx, wy = (hp[:, 0] + org[0]) / T(np.float32(CHECKER)), (hp[:, 1] + org[1]) / T(np.float32(CHECKER))
    par = (np.floor(wx).astype(np.int64) + np.floor(wy).astype(np.int64)) % 2
    near = th_ < T(np.float32(CHECKER_FAR))
    parity = np.where(gnd, np.where(near, par, 2), -1)
    chk = np.asarray(COL_CHK, np.float32).astype(T)
    alb = np.where((gnd & near)[:, None], chk[np.clip(par, 0, 1)], np.asarray(COL_FAR, np.float32).astype(T)[None, :])
    for k, pr in enumerate(prims):
        if pr is not None:
            alb = np.where(((best == k) & ~gnd)[:, None], pr[4][None, :], alb)
    ndl = _dot(nh, sun[None, :])
    lit = hit & (ndl > 0)
    so = hp + T(np.float32(SHADOW_EPS)) * nh
    idx = np.nonzero(lit)[0]
    if idx.size:
        sd = np.broadcast_to(sun, (idx.size, 3)).astype(T)
        blocked = np.zeros(idx.size, bool)
        for pr in prims:
            if pr is not None:
                blocked |= np.isfinite(_hit(pr, so[idx], sd, T)[0])
        lit[idx] = ~blocked
    shade = T(np.float32(AMBIENT)) + T(np.float32(DIFFUSE)) * np.maximum(ndl, 0) * lit.astype(T)
    col = alb * shade[:, None]
    s = np.clip(T(0.5) + T(0.5) * d[:, 2], 0, 1)
    sky = (1 - s)[:, None] * np.asarray(COL_HORIZON, np.float32).astype(T) + s[:, None] * np.asarray(COL_ZENITH, np.float32).astype(T)
    col = np.where(hit[:, None], col, sky)
    val = T(255) * np.clip(col, 0, 1) + T(0.5)   # rgb = floor(val); its distance to an integer is the rounding margin
    rgb = np.floor(val).astype(np.uint8)
    ids = np.where(gnd, ID_GROUND, np.where(best >= 0, best, ID_SKY)).astype(np.int32)
    depth = np.where(hit, th_, inf)
    sh = (Hh, W)
    return dict(rgb=rgb.reshape(Hh, W, 3), val=val.reshape(Hh, W, 3), id=ids.reshape(sh), depth=depth.reshape(sh),
                parity=parity.reshape(sh), lit=lit.reshape(sh))


def sensitive(view: View, base: dict | None = None, eps: float = 1.0 / 256.0) -> np.ndarray:
    """(H, W) bool: the float64 reference's discrete signature (id, checker parity, lit flag) changes when the pixel
    centre moves by +-eps pixel in x or in y."""
    b = base if base is not None else render(view, np.float64)
    out = np.zeros(b["id"].shape, bool)
    for sx, sy in ((eps, 0), (-eps, 0), (0, eps), (0, -eps)):
        r = render(view, np.float64, (sx, sy))
        out |= (r["id"] != b["id"]) | (r["parity"] != b["parity"]) | (r["lit"] != b["lit"])
    return out
