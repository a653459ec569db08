"""Inputs and float64 references for the evaluation and training-data kernels
(csrc/evaluate.hip marching cubes, ray caster and nearest neighbour;
csrc/train.hip k_mesh_sd), shared by test_eval_cases_host.py (CPU: the inputs
satisfy their conditions) and test_gpu_eval_kernels.py (GPU: the kernels equal
the references).  numpy only: nothing here touches a torch device or the code
under test.

References: oracle/marching_cubes.py, oracle.train.signed_distance, a float64
Moller-Trumbore brute force that rejects det == 0 and nothing else, and a
float64 all-pairs minimum.  Every input is built from a fixed seed and every
result is cached, so the tests of one run share one copy; callers must not
write into what they get."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

# ---------------------------------------------------------------------------
# marching cubes
# ---------------------------------------------------------------------------
MC_SHAPES = [(3, 5, 7), (7, 3, 5), (2, 9, 4), (17, 2, 3), (2, 2, 2), (33, 6, 9)]
MC_ISO_SHAPE = (7, 3, 5)
MC_ISOS = [0.37, -0.25]


def mc_noise_volume(shape):
    """Seeded randn with no outside border: surfaces cut the volume faces."""
    seed = shape[0] * 10000 + shape[1] * 100 + shape[2]
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def mc_corner_case(case: int):
    """2x2x2 volume of +-1 whose cube is case `case`: corner c (mc_table.CORNERS)
    is inside (value < 0) when bit c is set."""
    from tropical.utils.mc_table import CORNERS
    v = np.ones((2, 2, 2), np.float32)
    for c, (x, y, z) in enumerate(CORNERS):
        if (case >> c) & 1:
            v[x, y, z] = -1.0
    return v


def mc_case_strip():
    """The 256 case volumes side by side along x, [512, 2, 2]: cube 2 c is
    case c, the odd cubes between them are whatever two neighbours make."""
    return np.concatenate([mc_corner_case(c) for c in range(256)], 0)


def mc_table_count(case: int) -> int:
    from tropical.utils.mc_table import case_table
    return int((case_table()[case] >= 0).sum()) // 3


def mc_on_level_volume():
    """Samples drawn from {-1, 0, +0.0, -0.0, 1}: with iso = 0 neither zero is
    inside (-0.0 < 0 is false) and t is exactly 0, 1/2 or 1."""
    rs = np.random.RandomState(11)
    vals = np.array([-1.0, 0.0, +0.0, -0.0, 1.0], np.float32)
    return vals[rs.randint(0, 5, (8, 7, 9))]


def mc_empty_volumes():
    """(name, volume, iso): nothing crosses the level."""
    s = (4, 3, 5)
    return [("all_inside", np.full(s, -1.0, np.float32), 0.0),
            ("all_outside", np.full(s, 1.0, np.float32), 0.0),
            ("constant_on_level", np.full(s, 0.37, np.float32), 0.37)]


def mc_reference(vol, iso):
    from oracle.marching_cubes import marching_cubes
    from tropical.utils.mc_table import case_table
    return marching_cubes(vol, iso, case_table())


def degenerate_have_twin_vertices(V, F):
    """Every zero-area triangle of (V, F) has two identical vertices."""
    t = V[F]
    area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=-1)
    t = t[area == 0]
    twin = (t[:, 0] == t[:, 1]).all(1) | (t[:, 1] == t[:, 2]).all(1) | (t[:, 0] == t[:, 2]).all(1)
    return int((area == 0).sum()), bool(twin.all())


# ---------------------------------------------------------------------------
# ray caster
# ---------------------------------------------------------------------------
RAY_MARGIN = 1e-6   # band around a triangle's boundary (u, v, 1 - u - v, t) that excludes a ray
RAY_BAND = 1e-4     # a reported face must be a float64 hit of that face within this barycentric band
RAY_RTOL, RAY_ATOL = 1e-4, 1e-5  # depth: rtol, atol * L
RAY_N = 500


@lru_cache(maxsize=None)
def ray_mesh(name):
    """float32 vertices, int64 faces."""
    if name in ("noise", "thin"):
        v = np.random.RandomState(0).randn(12, 12, 12).astype(np.float32)
        v[0] = v[-1] = v[:, 0] = v[:, -1] = v[:, :, 0] = v[:, :, -1] = 1.0
        V, F = mc_reference(v, 0.0)
        V = (V / 11.0 * 2 - 1).astype(np.float32)
        if name == "thin":
            V = V * np.array([1, 1, 0.01], np.float32)
        return V, F
    if name == "planar":  # 8 x 8 quads over [-1, 1]^2 at z = 0.25, extent 0 on z
        g = np.linspace(-1, 1, 9)
        x, y = np.meshgrid(g, g, indexing="ij")
        V = np.stack([x.ravel(), y.ravel(), np.full(81, 0.25)], 1).astype(np.float32)
        F = []
        for i in range(8):
            for j in range(8):
                a, b, c, d = i * 9 + j, (i + 1) * 9 + j, (i + 1) * 9 + j + 1, i * 9 + j + 1
                F += [(a, b, c), (a, c, d)]
        return V, np.asarray(F, np.int64)
    if name == "triangle":
        return (np.array([[-0.6, -0.5, 0.1], [0.7, -0.3, -0.2], [0.1, 0.8, 0.3]], np.float32),
                np.array([[0, 1, 2]], np.int64))
    if name == "empty":
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    raise KeyError(name)


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _rays_inside(rs, n):
    return rs.rand(n, 3) * 0.4 - 0.2, _unit(rs.randn(n, 3))


def _rays_outside(rs, n):
    d = _unit(rs.randn(n, 3))
    return -3 * d + (rs.rand(n, 3) - 0.5) * 0.6, d


def _rays_mixed(rs, n):
    o1, d1 = _rays_inside(rs, n // 2)
    o2, d2 = _rays_outside(rs, n - n // 2)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def _rays_axis(rs, n):
    """From outside the box along +-e_a: two components are exactly +0.0."""
    o = rs.rand(n, 3) * 1.8 - 0.9
    d = np.zeros((n, 3))
    a, sg = rs.randint(0, 3, n), rs.choice([-1.0, 1.0], n)
    o[np.arange(n), a] = -2 * sg
    d[np.arange(n), a] = sg
    return o, d


def _rays_signed_zero(rs, n):
    """One component of every direction is -0.0, +0.0, 1e-30 or -1e-30."""
    o, d = _rays_mixed(rs, n)
    a = rs.randint(0, 3, n)
    z = np.array([-0.0, 0.0, 1e-30, -1e-30])[rs.randint(0, 4, n)]
    d[np.arange(n), a] = z
    o[n // 2:] = -3 * d[n // 2:] + (rs.rand(n - n // 2, 3) - 0.5) * 0.6
    return o, d


def _rays_nonunit(rs, n):
    o, d = _rays_mixed(rs, n)
    d[0::2] *= 0.01
    d[1::2] *= 100.0
    return o, d


def _rays_miss_box(rs, n):
    """From 3 units out, pointing away or tangentially: the box's corners are
    sqrt(3) from the centre, so every ray misses it."""
    u = _unit(rs.randn(n, 3))
    d = _unit(np.cross(u, rs.randn(n, 3)))
    d[0::2] = _unit(u[0::2] + 0.3 * rs.randn(len(u[0::2]), 3))
    return 3 * u, d


def _rays_steep(rs, n, z0=0.0):
    sg = rs.choice([-1.0, 1.0], n)
    o = np.concatenate([rs.rand(n, 2) * 1.8 - 0.9, (z0 - 2 * sg)[:, None]], 1)
    d = _unit(np.concatenate([0.2 * rs.randn(n, 2), sg[:, None]], 1))
    return o, d


def _rays_grazing(rs, n, z0=0.0):
    """Towards a point near the mesh with d_z scaled by 0.02 (not renormalised)."""
    d = _unit(rs.randn(n, 3))
    d[:, 2] *= 0.02
    target = np.concatenate([rs.rand(n, 2) * 1.6 - 0.8, np.full((n, 1), z0)], 1)
    return target - 3 * d, d


def _rays_triangle(rs, n):
    """Half towards random interior points of the single triangle (never its
    vertices or edge midpoints), half in random directions."""
    V, _ = ray_mesh("triangle")
    w = rs.dirichlet([1, 1, 1], n)
    target = w @ V.astype(np.float64)
    o = 2 * _unit(rs.randn(n, 3))
    d = _unit(target - o)
    d[1::2] = _unit(rs.randn(len(d[1::2]), 3))
    return o, d


# family: (mesh, generator, seed, scale, shift)
_RAY_FAMILIES = {
    "inside": ("noise", _rays_inside, 0, 1.0, 0.0),
    "outside": ("noise", _rays_outside, 1, 1.0, 0.0),
    "axis": ("noise", _rays_axis, 2, 1.0, 0.0),
    "signed_zero": ("noise", _rays_signed_zero, 3, 1.0, 0.0),
    "nonunit": ("noise", _rays_nonunit, 4, 1.0, 0.0),
    "miss_box": ("noise", _rays_miss_box, 5, 1.0, 0.0),
    "shift100": ("noise", _rays_mixed, 6, 1.0, 100.0),
    "scale1e-3": ("noise", _rays_mixed, 7, 1e-3, 0.0),
    "scale1e-5": ("noise", _rays_mixed, 7, 1e-5, 0.0),
    "scale1e3": ("noise", _rays_mixed, 7, 1e3, 0.0),
    "thin_steep": ("thin", _rays_steep, 8, 1.0, 0.0),
    "thin_grazing": ("thin", _rays_grazing, 9, 1.0, 0.0),
    "planar_steep": ("planar", lambda rs, n: _rays_steep(rs, n, 0.25), 10, 1.0, 0.0),
    "planar_grazing": ("planar", lambda rs, n: _rays_grazing(rs, n, 0.25), 11, 1.0, 0.0),
    "triangle": ("triangle", _rays_triangle, 12, 1.0, 0.0),
}
RAY_FAMILIES = list(_RAY_FAMILIES)


def ray_table(V, F, o, d, chunk=64):
    """float64 Moller-Trumbore of every ray against every triangle:
    (u, v, t, ok) as [R, F] arrays; ok = (det != 0), the only rejection."""
    V, o, d = V.astype(np.float64), o.astype(np.float64), d.astype(np.float64)
    a = V[F[:, 0]]
    e1, e2 = V[F[:, 1]] - a, V[F[:, 2]] - a
    out = [np.empty((len(o), len(F))) for _ in range(3)] + [np.empty((len(o), len(F)), bool)]
    for r0 in range(0, len(o), chunk):
        sl = slice(r0, r0 + chunk)
        dd = d[sl, None, :]
        p = np.cross(dd, e2[None])
        det = (e1[None] * p).sum(-1)
        ok = det != 0
        inv = 1.0 / np.where(ok, det, 1.0)
        s = o[sl, None, :] - a[None]
        q = np.cross(s, e1[None])
        out[0][sl] = (s * p).sum(-1) * inv
        out[1][sl] = (q * dd).sum(-1) * inv
        out[2][sl] = (q * e2[None]).sum(-1) * inv
        out[3][sl] = ok
    return tuple(out)


def classify_rays(V, F, o, d, m=RAY_MARGIN):
    """The float64 answer for every ray and whether it can be trusted.

    A triangle is hit clearly when u, v, 1 - u - v and t are all >= m, and
    hit in the band when they are all > -m but not all >= m.  A ray with a
    band hit on any triangle is excluded; the others are clear.  Returns
    excluded [R], t1 / f1 (nearest clear hit: inf / -1 when none) and t2 (the
    nearest clear hit on another face, inf when none)."""
    R = len(o)
    if len(F) == 0:
        return SimpleNamespace(excluded=np.zeros(R, bool), t1=np.full(R, np.inf), f1=np.full(R, -1),
                               t2=np.full(R, np.inf))
    u, v, t, ok = ray_table(V, F, o, d)
    lo = np.minimum(np.minimum(u, v), np.minimum(1 - u - v, t))
    clear = ok & (lo >= m)
    band = ok & (lo > -m) & ~clear
    tc = np.where(clear, t, np.inf)
    f1 = tc.argmin(1)
    t1 = tc[np.arange(R), f1]
    tc[np.arange(R), f1] = np.inf
    t2 = tc.min(1)
    return SimpleNamespace(excluded=band.any(1), t1=t1, f1=np.where(np.isfinite(t1), f1, -1), t2=t2)


def ray_face_hit(V, F, o, d, f):
    """(u, v, w, t) in float64 of ray r against its own face f[r]."""
    V, o, d = V.astype(np.float64), o.astype(np.float64), d.astype(np.float64)
    a = V[F[f, 0]]
    e1, e2 = V[F[f, 1]] - a, V[F[f, 2]] - a
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    s = o - a
    q = np.cross(s, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v, t = (s * p).sum(-1) / det, (q * d).sum(-1) / det, (q * e2).sum(-1) / det
    return u, v, 1 - u - v, t


@lru_cache(maxsize=None)
def _ray_base(mesh, seed):
    """The base rays of a seed (one generator per seed) and their classification."""
    V, F = ray_mesh(mesh)
    gen = next(g for (m, g, s, _, _) in _RAY_FAMILIES.values() if (m, s) == (mesh, seed))
    o, d = gen(np.random.RandomState(seed), RAY_N)
    o, d = o.astype(np.float32), d.astype(np.float32)
    return o, d, classify_rays(V, F, o, d)


@lru_cache(maxsize=None)
def ray_family(name):
    """One family: the float32 inputs the kernel gets (V, F, o, d: the base
    geometry scaled and shifted), the float64 classification of the base
    (unscaled, unshifted) geometry with its depths carried to the family's
    scale, and the depth tolerance's length L."""
    mesh, gen, seed, scale, shift = _RAY_FAMILIES[name]
    V0, F = ray_mesh(mesh)
    o0, d, ref = _ray_base(mesh, seed)
    V = (V0.astype(np.float64) * scale + shift).astype(np.float32)
    o = (o0.astype(np.float64) * scale + shift).astype(np.float32)
    if scale != 1.0:
        L = scale
    else:
        L = max(1.0, float(np.abs(o).max()), float(np.abs(V).max()) if len(V) else 0.0)
    return SimpleNamespace(name=name, V=V, F=F, o=o, d=d, V0=V0, o0=o0, scale=scale, shift=shift, L=L,
                           excluded=ref.excluded, f1=ref.f1, t1=ref.t1 * scale, t2=ref.t2 * scale)


def ray_tol(fam, t):
    return RAY_RTOL * np.abs(t) + RAY_ATOL * fam.L


# ---------------------------------------------------------------------------
# nearest neighbour
# ---------------------------------------------------------------------------
NN_SIZES = [(1, 1), (3, 5), (1, 1025), (255, 1023), (256, 1024), (257, 1025), (1000, 2049)]
NN_RTOL, NN_ATOL = 1e-5, 1e-6  # atol * L


def nn_reference(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.sqrt(((a[:, None, :] - b[None]) ** 2).sum(-1)).min(1)


def nn_clouds(na, nb, seed=None):
    rs = np.random.RandomState(na * 7919 + nb if seed is None else seed)
    return rs.rand(na, 3).astype(np.float32), rs.rand(nb, 3).astype(np.float32)


def nn_length(a, b):
    """L of the tolerance: the largest absolute coordinate, floored at 1."""
    return max(1.0, float(np.abs(a).max()) if a.size else 0.0, float(np.abs(b).max()) if b.size else 0.0)


@lru_cache(maxsize=None)
def nn_case(name):
    """(a, b) float32 for the named special case."""
    if name == "own_rows":  # every a is a row of b: the distance is exactly 0
        a, b = nn_clouds(300, 1500, 21)
        return b[np.random.RandomState(22).randint(0, 1500, 300)].copy(), b
    if name == "shift100":
        a, b = nn_clouds(257, 1025, 23)
        return a + np.float32(100), b + np.float32(100)
    if name == "outlier":  # one far point in the middle of the second tile
        a, b = nn_clouds(257, 2049, 24)
        b = b.copy()
        b[1500] = (50.0, -40.0, 30.0)
        return a, b
    raise KeyError(name)


# ---------------------------------------------------------------------------
# mesh signed distance
# ---------------------------------------------------------------------------
SD_RADIUS = 0.8
SD_MAG_TOL = 2e-6    # * max(1, |ref|)
SD_SIGN_MIN = 1e-4   # the sign is compared where |ref| is above this ...
SD_WIND_GAP = 0.05   # ... and the float64 winding number is this far from +-0.5
SD_TILE, SD_BLOCK = 256, 256  # csrc/train.hip SD_TILE, common.h TNP_BLOCK


def sd_launch_shape(n, nF):
    """launch_mesh_sd's grid restated: (bx, by, sizes of the by chunks)."""
    bx = (n + SD_BLOCK - 1) // SD_BLOCK
    by = max(1, min((nF + SD_TILE - 1) // SD_TILE, (2048 + bx - 1) // bx))
    chunk = ((nF + by - 1) // by + SD_TILE - 1) // SD_TILE * SD_TILE
    by = (nF + chunk - 1) // chunk
    return bx, by, [min(chunk, nF - i * chunk) for i in range(by)]


def _icosphere(level):
    from test_train import icosphere
    V, F = icosphere(level, r=SD_RADIUS)
    return V.astype(np.float32), F


def _edges(F):
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), 1)
    return np.unique(e, axis=0)


def _with_degenerates(V, F, n_edges=3, fractions=((0.5, 0.3, 0.7), (0.5, 0.3, 0.7), (0.5, 0.3))):
    """Append degenerate triangles lying on the mesh's own edges: per edge
    (a, b) every arrangement of (a, a, b) and (a, b, b), then (a, a, a), then
    (a, m, b) in its three rotations for inserted points m on the edge."""
    V = [v for v in V.astype(np.float64)]
    extra = []
    E = _edges(F)
    for (a, b), fr in zip(E[:: len(E) // n_edges][:n_edges], fractions):
        a, b = int(a), int(b)
        extra += [(a, a, b), (a, b, a), (b, a, a), (a, b, b), (b, a, b), (b, b, a), (a, a, a)]
        for f in fr:
            V.append(V[a] + f * (V[b] - V[a]))
            m = len(V) - 1
            extra += [(a, m, b), (m, b, a), (b, a, m)]
    return np.asarray(V).astype(np.float32), np.concatenate([F, np.asarray(extra, np.int64)])


@lru_cache(maxsize=None)
def sd_mesh(name):
    """float32 vertices, int64 faces."""
    if name == "sphere80":
        return _icosphere(1)
    if name == "sphere":
        return _icosphere(2)
    if name == "flipped":
        V, F = _icosphere(2)
        return V, F[:, ::-1].copy()
    if name == "hemisphere":  # open: the faces above the equator
        V, F = _icosphere(2)
        return V, F[V[F][:, :, 2].mean(1) > 0]
    if name == "triangle":
        return ray_mesh("triangle")
    if name == "sphere_degenerate":  # 320 + 45
        return _with_degenerates(*_icosphere(2))
    if name == "sphere1325":        # 1280 + 45: three chunks of two tiles, the last one partial
        return _with_degenerates(*_icosphere(3))
    raise KeyError(name)


@lru_cache(maxsize=None)
def sd_points(kind):
    """float32 points around the 320-face sphere."""
    V, F = _icosphere(2)
    V = V.astype(np.float64)
    rs = np.random.RandomState(31)
    E = _edges(F)
    mid = (V[E[:, 0]] + V[E[:, 1]]) / 2
    tri = V[F]
    cen = tri.mean(1)
    nrm = _unit(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
    if kind == "random":
        P = rs.rand(3000, 3) * 2.4 - 1.2
    elif kind == "on_features":   # magnitude only: the sign is undefined on the surface
        P = np.concatenate([V, mid, cen])
    elif kind == "off_features":
        P = np.concatenate([V * 1.2, V * 0.8, mid + 0.2 * _unit(mid), mid - 0.2 * _unit(mid),
                            cen + 0.1 * nrm, cen - 0.1 * nrm, cen + 1e-3 * nrm, cen - 1e-3 * nrm])
    elif kind == "far":
        P = 30 * _unit(rs.randn(300, 3)) + rs.randn(300, 3)
    elif kind == "all":
        return np.concatenate([sd_points(k) for k in ("random", "on_features", "off_features", "far")])
    else:
        raise KeyError(kind)
    return P.astype(np.float32)


def sd_sign_ok_mask(n):
    """Points of sd_points('all') whose sign is compared (not the on-feature ones)."""
    k = [len(sd_points(x)) for x in ("random", "on_features", "off_features", "far")]
    m = np.ones(sum(k), bool)
    m[k[0]:k[0] + k[1]] = False
    assert len(m) == n
    return m


@lru_cache(maxsize=None)
def sd_big_points():
    """200 000 points for the 1325-face mesh, and the indices the oracle runs
    on: the first block, the last block and every 101st point between."""
    n = 200000
    P = (np.random.RandomState(32).rand(n, 3) * 2.4 - 1.2).astype(np.float32)
    idx = np.concatenate([np.arange(SD_BLOCK), np.arange(SD_BLOCK, n - SD_BLOCK, 101), np.arange(n - SD_BLOCK, n)])
    return P, idx


@lru_cache(maxsize=None)
def sd_reference(mesh, points):
    """(signed distance, winding number) of oracle.train.signed_distance on
    the same float32 (V, F) the kernel gets."""
    from oracle.train import signed_distance
    V, F = sd_mesh(mesh)
    if points == "big":
        P, idx = sd_big_points()
        P = P[idx]
    elif isinstance(points, int):
        P = sd_points("random")[:points]
    else:
        P = sd_points(points)
    with np.errstate(divide="ignore", invalid="ignore"):
        return signed_distance(V, F, P)


def sd_regions(V, F, P):
    """Which feature of its nearest triangle is nearest to every point, in
    float64: 0, 1, 2 = vertex a, b, c; 3, 4, 5 = edge ab, bc, ca; 6 = face
    (in the triangle's own vertex order, the order tri_dist2 sees).  Ties
    between triangles go to the first."""
    V, P = V.astype(np.float64), P.astype(np.float64)
    best = np.full(len(P), np.inf)
    region = np.full(len(P), -1)
    for f in F:
        a, b, c = V[f[0]], V[f[1]], V[f[2]]
        ab, ac = b - a, c - a
        n = np.cross(ab, ac)
        nn = n @ n
        if nn == 0:
            continue
        ap = P - a
        v = np.cross(ap, ac) @ n / nn
        w = np.cross(ab, ap) @ n / nn
        inside = (v >= 0) & (w >= 0) & (v + w <= 1)
        proj = a + v[:, None] * ab + w[:, None] * ac
        d2 = np.where(inside, ((P - proj) ** 2).sum(1), np.inf)
        reg = np.where(inside, 6, -1)
        for k, (p0, p1, v0, v1) in enumerate(((a, b, 0, 1), (b, c, 1, 2), (c, a, 2, 0))):
            e = p1 - p0
            t = np.clip((P - p0) @ e / (e @ e), 0, 1)
            de = ((P - (p0 + t[:, None] * e)) ** 2).sum(1)
            r = np.where(t == 0, v0, np.where(t == 1, v1, 3 + k))
            better = de < d2
            d2, reg = np.where(better, de, d2), np.where(better, r, reg)
        better = d2 < best
        best, region = np.where(better, d2, best), np.where(better, reg, region)
    return region
