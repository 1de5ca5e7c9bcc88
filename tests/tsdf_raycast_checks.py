"""Checks of the TSDF ray cast whose bounds come from geometry, not from the code under test (shared by
tests/test_tsdf_raycast_api.py: the numpy reference and the serial program; tests/test_gpu_tsdf_raycast.py: the kernel).  Each check
takes cast(volume, params, view) -> dict(depth, normals, status) and returns the measured maxima next to the derived bounds.

Notation.  h = voxel, tau = trunc, Q = 32767, u = tau / Q (one unit of t in metres), q = u / 2 (the quantisation of a stored t),
eps = 2^-24.  A ray is X(Z) = c + Z * dw with dw = transpose(R) * (dx, dy, 1), |dw| >= 1; phi is the true signed distance, n its unit
gradient at the intersection Z*, s = |n . dw| = |d phi / dZ| there; cos = s / |dw| is the cosine of ray against normal.

Binary32 allowance (stated, not measured).  A sample's grid coordinate g = g0 + Z * gd comes out of at most 16 roundings of
quantities no larger than G = max(|g0|) + z_far * max(|gd|) grid units (the products and sums of the rotation, the camera centre, the
scale by inv_voxel, the sample itself), so it lies within 16 * eps * G of its real value per axis, sqrt(3) times that in space;
phi is 1-Lipschitz, so the field seen moves by at most r_pos = sqrt(3) * 16 * eps * G * h metres.  The seven lerps of the interpolant
round 21 times on magnitudes <= Q: r_lerp = 32 * eps * Q * u.  The hit depth is three more roundings at magnitude <= z_far:
r_z = 4 * eps * z_far.

Plane.  phi is linear, the trilinear interpolant reproduces a linear function exactly and is a convex combination of its corners, so
wherever all eight corners are unsaturated the interpolated field is phi + e with |e| <= q.  The two samples around the crossing are
such (tau is chosen > step * |dw| + sqrt(3) * h), and a free sample, at least tau - 0.87 * h from the surface, cannot skip past it
(tau - 0.87 * h - skip * |dw| > 0).  The march's linear interpolation between them is a line g(Z) = phi(Z) + e(Z),
|e| <= q + r_pos + r_lerp on the interval, so its zero Zh satisfies |phi(Zh)| <= q + r_pos + r_lerp, hence
    |Zh - Z*| <= (q + r_pos + r_lerp) / s + r_z.
Normal: a corner difference along an axis is h * n_axis / u + d in units of t with |d| <= 1 (two half units) + 0.05 (roundings), the
blend of four of them the same, so the gradient is M * n + d with M = h / u and |d| <= 1.05 * sqrt(3); normalising at most doubles the
relative error: every component of the unit normal lies within 2 * 1.05 * sqrt(3) / M + 1e-6 of R * n (1e-6: the rotation's roundings).

Sphere (radius r, rho_min = r - (step * |dw|max + sqrt(3) * h): the least distance from the centre of any corner used near the
surface).  The Hessian of phi = |X - C| - r is positive semidefinite with eigenvalues 0, 1/rho, 1/rho, so its diagonal entries are
non-negative and sum to 2 / rho.  Trilinear interpolation on a cell of edge h errs by at most (h^2 / 8) * (|phi_xx| + |phi_yy| +
|phi_zz|) <= h^2 / (4 * rho_min) =: E_i.  Along the ray phi has a second derivative <= |dw|^2 / rho_min, so the chord between two samples
l = step apart in Z errs by at most step^2 * |dw|^2 / (8 * rho_min) =: E_c.  So |phi(Zh)| <= E = q + E_i + E_c + r_pos + r_lerp, and with
the slope of phi between Zh and Z* at least s_lb = s - step * |dw|^2 / rho_min:
    |Zh - Z*| <= E / s_lb + r_z.
Normal.  A component, say x, of the interpolant's gradient is the bilinear blend in (y, z) of the four corner differences along x over
h.  Each difference over h is the MEAN of phi_x along its edge.  Row x of the Hessian, (e_x - n_x n) / rho, is no longer than
1 / rho_min, so |phi_x(xi) - phi_x(p)| <= |xi - p| / rho_min for a point xi of an edge and the hit point p.  The blend's weights w_i
(they sum to 1) times the uniform measure on each edge is a probability measure, and by Jensen's inequality the mean of |xi - p| is
at most the root of the mean of |xi - p|^2: its x part is h^2 (1/3 - a + a^2) <= h^2 / 3 (a: the hit's fraction along x), its
weighted y and z parts are h^2 b (1 - b) and h^2 c (1 - c), at most h^2 / 4 each.  So every component of the
gradient is within e_c = sqrt(5/6) * h / rho_min + 2.1 * q / h of the true one (2.1 * q / h: two half units of t over h, and the
roundings), the gradient vector within D = sqrt(3) * e_c of the unit vector n(p).  Normalising a vector within D < 1 of a unit vector
turns it by an angle whose sine is at most D, so the unit vectors differ by at most D / sqrt(1 - D^2), and so does every component.
The true normal moves by |Zh - Z*| * |dw| / rho_min between Zh and Z*.  Every component lies within
    D / sqrt(1 - D^2) + B_depth * |dw|max / rho_min + 1e-6        (1e-6: the rotation's roundings).

Round trip.  A voxel takes the depth D(B) of the pixel B its centre projects to, so the field along the ray of pixel A is built from
the depths of the pixels that the corners of A's cells project to: those within the voxel's footprint in pixels (voxel * focal / Z,
rounded up) plus the two pixels of the projection's rounding and the cell's reach.  Where the map changes by more than the model
resolves inside that neighbourhood -- a depth step: 4-neighbours further apart in depth than one voxel edge, or one of them without
depth -- the crossing along A's ray need not lie near D(A).  So a pixel is ruled out, from the input map alone, when it has no depth
or lies within `radius` pixels (Chebyshev) of a depth step or of the image border (beyond it the map has no depth either); radius = 2
where a voxel spans less than a pixel (the rule as the synthetic scene uses it), and footprint + 2 where it spans more.
"""
import numpy as np

from tests import tsdf_raycast_cases as RC
from tests import tsdf_raycast_ref as RR
from tests import tsdf_ref as T

F = np.float32
EPS = 2.0 ** -24
MIN_COS = 0.5  # the smallest |cos| of ray against normal at which a pixel is judged (none grazing)


def geometry(p, v):
    """float64, from the binary32 values of the parameters: camera centre c [3], directions dw [H][W][3], dx, dy"""
    R = np.asarray([F(x) for x in v["R"]], np.float64).reshape(3, 3)
    t = np.asarray([F(x) for x in v["t"]], np.float64)
    y, x = np.mgrid[0:v["height"], 0:v["width"]].astype(np.float64)
    d = np.stack([(x - float(F(v["cx"]))) / float(F(v["focal_px"])), (y - float(F(v["cy"]))) / float(F(v["focal_px"])), np.ones_like(x)], -1)
    return -(R.T @ t), d @ R, R  # (d @ R = transpose(R) * d per pixel)


def grid_of(p, X):
    return (X - np.asarray([float(F(o)) for o in p["origin"]])) / float(F(p["voxel"])) - 0.5


def allowances(p, v, c, dw):
    h, u = float(F(p["voxel"])), float(F(p["trunc"])) / T.Q
    G = np.abs(grid_of(p, c)).max() + float(F(v["z_far"])) * np.abs(dw).max() / h
    return dict(h=h, u=u, q=u / 2, r_pos=np.sqrt(3) * 16 * EPS * G * h, r_lerp=32 * EPS * T.Q * u, r_z=4 * EPS * float(F(v["z_far"])))


def inner(p, X, margin=1.0):
    """the point lies inside the box of centres, more than `margin` cells from its boundary"""
    g = grid_of(p, X)
    n = np.asarray([p["nx"], p["ny"], p["nz"]], np.float64)
    return ((g > margin) & (g < n - 1 - margin)).all(-1)


def judge(p, v, out, Zs, nw, bound_depth, bound_normal, must_hit):
    """Zs: analytic depth (nan: none); nw: analytic world normal [H][W][3]; must_hit: pixels that have to be HIT -> measured maxima"""
    c, dw, R = geometry(p, v)
    hit = out["status"] == RR.HIT
    assert (hit | ~must_hit).all(), "%d rays that meet the surface well inside the box are no HIT" % int((must_hit & ~hit).sum())
    judged = hit & must_hit
    assert judged.sum() > 0
    err_z = np.abs(out["depth"].astype(np.float64) - Zs)
    nc = nw @ R.T
    err_n = np.abs(out["normals"][..., :3].astype(np.float64) - nc).max(-1)
    bd = np.broadcast_to(bound_depth, err_z.shape)
    assert (err_z[judged] <= bd[judged]).all(), ("depth", float(err_z[judged].max()), float(bd[judged].min()))
    assert (err_n[judged] <= bound_normal).all(), ("normal", float(err_n[judged].max()), bound_normal)
    assert (out["normals"][..., 2][judged] < 0).all()  # (the surface faces the camera: the sign convention of adc_normals)
    return dict(judged=int(judged.sum()), depth=float(err_z[judged].max()), depth_bound=float(bd[judged].max()), depth_share=float((err_z[judged] / bd[judged]).max()),
                normal=float(err_n[judged].max()), normal_bound=float(bound_normal))


# ---------------------------------------------------------------------------------------------- plane
PLANE_N, PLANE_C = (0.12, -0.2, 1.0), 0.93
PLANE_POSES = ((T.IDENTITY, (0.0, 0.0, 0.0)), (RC.TC.rot(12.0, -17.0, 25.0), (0.2, -0.15, 0.1)), (RC.TC.rot(-20.0, 9.0, -8.0), (-0.12, 0.3, 0.15)))


def plane_volume():
    p = T.params(16, 20, 24, 0.04, (-0.32, -0.4, 0.5), 0.16)
    return p, RC.field_volume(p, RC.plane(PLANE_N, PLANE_C))


def check_plane(cast, pose_index, skip_factor=1.0):
    p, vol = plane_volume()
    R, t = RC.pose(*PLANE_POSES[pose_index])
    v = RR.view(41, 29, 38.0, 20.3, 14.1, R, t, z_near=0.1, z_far=4.0, step=0.02, skip=0.02 * skip_factor)
    out = cast(vol, p, v)
    c, dw, _ = geometry(p, v)
    n = np.asarray(PLANE_N) / np.linalg.norm(PLANE_N)
    sgn = -1.0  # phi = (C - N . X) / |N|: its gradient is -n
    s = np.abs(dw @ n)
    Zs = (PLANE_C / np.linalg.norm(PLANE_N) - c @ n) / (dw @ n)
    cos = s / np.linalg.norm(dw, axis=-1)
    a = allowances(p, v, c, dw)
    far = np.linalg.norm(dw, axis=-1).max()
    assert float(F(p["trunc"])) > float(F(v["step"])) * far + np.sqrt(3) * a["h"]  # (the samples around the crossing are unsaturated)
    assert float(F(p["trunc"])) - 0.87 * a["h"] - float(F(v["skip"])) * far > 0       # (a free sample's skip cannot pass the surface)
    must = (Zs > v["z_near"]) & (Zs < v["z_far"]) & inner(p, c + Zs[..., None] * dw) & (cos >= MIN_COS)
    bound_z = (a["q"] + a["r_pos"] + a["r_lerp"]) / s + a["r_z"]
    bound_n = 2 * 1.05 * np.sqrt(3) / (a["h"] / a["u"]) + 1e-6
    m = judge(p, v, out, Zs, np.broadcast_to(sgn * n, dw.shape), bound_z, bound_n, must)
    m["min_cos"] = float(cos[must].min())
    return m


# ---------------------------------------------------------------------------------------------- sphere
SPHERE_C, SPHERE_R = (0.01, -0.02, 1.0), 0.3
SPHERE_VOXELS = (0.04, 0.02, 0.0125)


def sphere_volume(h):
    n = int(round(0.8 / h))
    n += -n % 4
    p = T.params(n, n, n, h, (SPHERE_C[0] - n * h / 2, SPHERE_C[1] - n * h / 2, SPHERE_C[2] - n * h / 2), 4 * h)
    return p, RC.field_volume(p, RC.sphere(SPHERE_C, SPHERE_R))


def check_sphere(cast, h):
    p, vol = sphere_volume(h)
    R, t = RC.pose(RC.TC.rot(5.0, -7.0, 11.0), (0.08, -0.05, 0.0))
    v = RR.view(45, 33, 50.0, 22.0, 16.0, R, t, z_near=0.1, z_far=3.0, step=h / 2, skip=h / 2)
    out = cast(vol, p, v)
    c, dw, _ = geometry(p, v)
    C = np.asarray(SPHERE_C)
    oc = c - C
    A, B, Cc = (dw * dw).sum(-1), 2 * (dw @ oc), oc @ oc - SPHERE_R ** 2
    with np.errstate(all="ignore"):
        Zs = (-B - np.sqrt(B * B - 4 * A * Cc)) / (2 * A)
    X = c + np.nan_to_num(Zs)[..., None] * dw
    nw = (X - C) / SPHERE_R
    norm = np.linalg.norm(dw, axis=-1)
    s = np.abs((nw * dw).sum(-1))
    cos = s / norm
    a = allowances(p, v, c, dw)
    step = float(F(v["step"]))
    rho = SPHERE_R - (step * norm.max() + np.sqrt(3) * a["h"])
    E = a["q"] + a["h"] ** 2 / (4 * rho) + step ** 2 * norm ** 2 / (8 * rho) + a["r_pos"] + a["r_lerp"]
    s_lb = s - step * norm ** 2 / rho
    must = np.isfinite(Zs) & (cos >= MIN_COS) & inner(p, X)
    with np.errstate(all="ignore"):
        bound_z = np.where(must, E / s_lb + a["r_z"], np.inf)
    assert (s_lb[must] > 0).all()
    D = np.sqrt(3) * (np.sqrt(5.0 / 6.0) * a["h"] / rho + 2.1 * a["q"] / a["h"])
    assert D < 1
    bound_n = D / np.sqrt(1 - D * D) + bound_z[must].max() * norm.max() / rho + 1e-6
    m = judge(p, v, out, np.where(must, Zs, 0.0), nw, bound_z, bound_n, must)
    m["voxel"] = h
    return m


# ---------------------------------------------------------------------------------------------- round trip with the integrator
def roundtrip_scene(W=80, H=60):
    """a tilted plane with a sphere standing between it and the camera (the other way round the sphere would be hidden), as the depth
    map of a pose P: (params, frame, depth map with +inf = none)"""
    calib = (70.0, 0.1, 39.5, 29.5, 0.0)
    R, t = RC.pose(RC.TC.rot(4.0, -6.0, 3.0), (0.05, -0.03, 0.0))
    surface_plane = RC.TC.plane_surface((0.1, -0.15, 1.0), 1.3)
    surface_sphere = RC.TC.sphere_surface((0.05, 0.0, 1.0), 0.15)

    def both(o, d):
        a, b = surface_plane(o, d), surface_sphere(o, d)
        return np.where(np.isfinite(b) & (b > 0), b, a)
    Z = RC.TC.raycast_depth(W, H, calib, R, t, both)
    Z[:4, :] = np.inf  # (pixels without depth)
    # a voxel spans 0.0125 * 70 / Z < 1 pixel everywhere in the scene (Z > 0.85): the corners of a sample's cell project within two
    # pixels of the ray's own pixel, which is what the two-pixel rule presumes
    p = T.params(136, 100, 64, 0.0125, (-0.625, -0.4825, 0.75), 0.05)
    return p, T.frame(calib, R, t, T.FROM_DEPTH), Z.astype(F), calib


def roundtrip_ruled_out(Z, step_threshold, radius=2):
    """From the input map alone (the module's docstring, Round trip): a pixel is ruled out when the input has no depth there, or within
    `radius` pixels (Chebyshev) of a depth step -- a pair of 4-neighbours whose depths differ by more than step_threshold, or of which
    one has no depth -- or of the image's border."""
    has = np.isfinite(Z) & (Z > 0)
    Zf = np.where(has, Z, 0.0).astype(np.float64)
    edge = np.zeros(Z.shape, bool)
    for ax in (0, 1):
        a = [slice(None)] * 2
        b = [slice(None)] * 2
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        jump = (has[a] != has[b]) | (has[a] & has[b] & (np.abs(Zf[a] - Zf[b]) > step_threshold))
        edge[a] |= jump
        edge[b] |= jump
    near = np.pad(edge, radius, constant_values=True)  # (a square neighbourhood: rows, then columns)
    for ax in (0, 1):
        acc = np.zeros_like(near)
        for d in range(-radius, radius + 1):
            acc |= np.roll(near, d, axis=ax)
        near = acc
    near = near[radius:-radius, radius:-radius]
    return ~has | near


def check_roundtrip(cast, integrate, frames=3):
    """integrate(volume, p, frame, map) -> volume; the pixels of the volume's outermost cells leave too (the model ends there)"""
    p, fr, Z, calib = roundtrip_scene()
    vol = T.empty(p)
    for _ in range(frames):
        vol = integrate(vol, p, fr, Z)
    H, W = Z.shape
    h = float(F(p["voxel"]))
    v = RR.view(W, H, calib[0], calib[2], calib[3], fr["R"], fr["t"], z_near=0.2, z_far=3.0, step=h / 2, skip=float(F(p["trunc"])) / 2)
    out = cast(vol, p, v)
    out_rule = roundtrip_ruled_out(Z, h)  # (a step: neighbours further apart in depth than the model resolves)
    c, dw, _ = geometry(p, v)
    inside = inner(p, c + np.where(np.isfinite(Z), Z, 0.0)[..., None].astype(np.float64) * dw, 2.0)
    judged = ~out_rule & inside
    share = float(out_rule.mean())
    hit = out["status"] == RR.HIT
    err = np.abs(out["depth"].astype(np.float64) - Z.astype(np.float64))
    print("round trip: %d of %d pixels ruled out by the input map (%.1f %%), %d outside the volume's inner cells, %d judged; HIT on %d of them; max |dZ| = %.5f m = %.3f voxel"
          % (out_rule.sum(), Z.size, 100 * share, int((~out_rule & ~inside).sum()), judged.sum(), int((hit & judged).sum()), float(err[judged & hit].max()), float(err[judged & hit].max()) / h))
    assert judged.sum() > 0.5 * Z.size
    assert (hit | ~judged).all(), int((judged & ~hit).sum())
    assert (err[judged] <= h).all(), float(err[judged].max())
    return dict(share=share, ruled_out=int(out_rule.sum()), judged=int(judged.sum()), depth=float(err[judged].max()), voxel=h)
