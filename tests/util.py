"""Helpers shared by the tests."""
import ctypes as C

import numpy as np

from rttnw_amd import abi
from rttnw_amd import scene as S


build, params_for = S.build, S.params_for  # (live in the package: bench.py and smoke() use them too)


def hostsim_render(hostsim, sc, cam, p, n_threads=0):
    lin = np.zeros((p.height, p.width, 3))
    st = abi.Stats()
    rc = hostsim.lib.hostsim_render(sc.handle, C.byref(cam), C.byref(p), lin.ctypes.data, C.byref(st), n_threads)
    assert rc == 0
    return lin, st


class LaunchPlanOut(C.Structure):
    """tests/hostsim/hostsim.cpp HostsimLaunchPlan: launch_plan.hpp's LaunchPlan as plain integers, and the scene's 4-wide node count."""
    _fields_ = [(n, C.c_uint32) for n in ("decoupled", "lds", "count", "list", "quantised", "shapes", "steps", "block", "lds_nodes")] + \
               [("lds_recs", C.c_uint32 * 6)] + [(n, C.c_uint32) for n in ("staged_bytes", "lds_bytes", "form_bits", "n_nodes")]

    def key(self, **replace):
        """The fields as a comparable tuple, some of them replaced."""
        d = {n: (tuple(getattr(self, n)) if n == "lds_recs" else getattr(self, n)) for n, _ in self._fields_}
        assert set(replace) <= set(d)
        d.update(replace)
        return tuple(sorted(d.items()))


def hostsim_launch_plan(lib, sc, real_bytes, count=0, listed=0, forced=0, wave_block=0):
    """The launch plan of a render of `sc` through the host build `lib` (a ctypes library).  forced: 0 auto, 1 plain, 2 plainglobal, 3 wave."""
    lib.hostsim_launch_plan.restype = C.c_int
    lib.hostsim_launch_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LaunchPlanOut)]
    out = LaunchPlanOut()
    assert lib.hostsim_launch_plan(sc.handle, real_bytes, count, listed, forced, wave_block, C.byref(out)) == 0
    return out


def block_means(rgb, n):
    h, w, _ = rgb.shape
    bh, bw = h // n, w // n
    return np.array([[[rgb[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw, ch].mean() for c in range(n)]
                      for r in range(n)] for ch in range(3)])


# ---- per-bounce path dumps: product (device probe kernel, or the host build of the same core) vs the oracle
PROBE_STRIDE = 20  # include/rttnw_hip.h rttnw_debug_probe_path


def product_probe(fn, binding, sc, cam, p, px, row, sample, max_out=64):
    """fn = gpu.debug_probe_path or hostsim.lib.hostsim_probe_path -> array [n_hits, 20]."""
    out = np.zeros(max_out * PROBE_STRIDE + 4, dtype=np.float64)
    n = fn(sc.handle, C.byref(cam), C.byref(p), px, row, sample, out.ctypes.data, max_out)
    abi.check(n, binding, "probe_path")
    return out[:n * PROBE_STRIDE].reshape(n, PROBE_STRIDE)


def compare_paths(probe, oracle_probe, pairs, tol=1e-9, growth=1.0):
    """Every bounce of every (px, row, sample): t, p, normal, front_face equal within `tol` (relative to the magnitude of
    the coordinate) AT EVERY DEPTH.  `growth` > 1 — only for the contracted build on the scenes whose small spheres amplify a last-place
    difference (the world-space test of a transformed group's spheres, a fused multiply-add: a different ray after the bounce, growing by
    ~(1 + distance / radius) per bounce, x10 in final_scene's cluster) — loosens the bound to tol x growth^(k - 2) at bounce k > 2, capped
    at 1e-4; RTTNW_F64_STRICT probes are held to 1e-12 flat (tests/test_gpu_parity.py).  The DECISIONS — front face, material,
    scattered or absorbed, bounce count — are exact at every depth; the same material at every hit (the oracle reports graph ids, the product flat indices: the
    mapping must be one-to-one and order preserving), (u, v) equal wherever the product computes them (it skips them
    when no texture reads them).  Returns (paths, bounces compared, material map)."""
    mat_map, bounces = {}, 0
    for (px, row, s) in pairs:
        a = probe(px, row, s)
        b = oracle_probe(px, row, s)
        assert len(a) == len(b), ("bounce count", px, row, s, len(a), len(b))
        for k in range(len(a)):
            scale = max(1.0, np.abs(b[k, 0:4]).max())
            tol_k = min(max(tol, 1e-4), tol * growth ** max(0, k - 2))
            assert np.abs(a[k, 0:7] - b[k, 0:7]).max() <= tol_k * scale, ("t/p/normal", px, row, s, k, a[k, 0:7], b[k, 0:7])
            assert a[k, 10] == b[k, 10], ("front_face", px, row, s, k)
            if a[k, 8] != 0.0 or a[k, 9] != 0.0:
                assert abs(a[k, 8] - b[k, 8]) <= tol_k and abs(a[k, 9] - b[k, 9]) <= tol_k, ("uv", px, row, s, k)
            assert mat_map.setdefault(int(b[k, 7]), int(a[k, 7])) == int(a[k, 7]), ("material", px, row, s, k)
            assert (a[k, 19] >= 0.0) == (b[k, 11] == 1.0), ("scattered", px, row, s, k)
            bounces += 1
    ids = sorted(mat_map)
    flat = [mat_map[i] for i in ids]
    assert flat == sorted(flat) and len(set(flat)) == len(flat), mat_map
    return len(pairs), bounces, mat_map


# ---- the re-anchored per-bounce tier: every bounce of the PRODUCT's path against the oracle's same operation AT THE PRODUCT'S INPUT
EPS_F32, EPS_F64 = 2.0 ** -24, 2.0 ** -53


def product_probe_tail(fn, binding, sc, cam, p, px, row, sample, max_out=64):
    """product_probe with the probe's tail: (records [n, 20], tail [4] = radiance r, g, b (black background) and bounce count)."""
    out = np.zeros(max_out * PROBE_STRIDE + 4, dtype=np.float64)
    n = fn(sc.handle, C.byref(cam), C.byref(p), px, row, sample, out.ctypes.data, max_out)
    abi.check(n, binding, "probe_path")
    return out[:n * PROBE_STRIDE].reshape(n, PROBE_STRIDE).copy(), out[max_out * PROBE_STRIDE:max_out * PROBE_STRIDE + 4].copy()


def _ray_perturbations(ray, eps, K, size=1.0):
    """The ray [7] and its 12 one-coordinate perturbations: origin by +-K eps max(|o|, size) per axis, direction by +-K eps |d|."""
    do = K * eps * max(np.abs(ray[0:3]).max(), size, 1.0)
    dd = K * eps * np.abs(ray[3:6]).max()
    out = [ray]
    for a in range(3):
        for sg in (-1.0, 1.0):
            r = ray.copy(); r[a] += sg * do; out.append(r)
            r = ray.copy(); r[3 + a] += sg * dd; out.append(r)
    return out


def _ball_is_ambiguous(seed, pixel, sample, bounce, band):
    """random_in_unit_space's rejection loop (the oracle's draw spec): True when a candidate up to the accepted one has |v|^2 within
    `band` of 1 — a build that rounds the candidate (f32: the top 24 of its 53 bits) may accept or reject it the other way."""
    from oracle import rto
    for it in range(64):
        c = rto.SLOT_SCATTER + 4 * it
        h, lo, mi = (rto.probe_word(seed, pixel, sample, bounce + 1, c + j) for j in range(3))
        fields = (h >> 43, (h >> 22) & 0x1FFFFF, (h >> 1) & 0x1FFFFF)
        lows = (lo >> 32, lo & 0xFFFFFFFF, mi >> 32)
        v = np.array([2.0 * float((f << 32) | l) / 9007199254740992.0 - 1.0 for f, l in zip(fields, lows)])
        sq = float(v @ v)
        if abs(sq - 1.0) <= band:
            return True
        if sq < 1.0:
            return False
    return False


def _sphere_uv(n):
    """hittable.rs:77-83 for the outward normal n."""
    return np.array([(np.arctan2(-n[2], n[0]) + np.pi) / (2.0 * np.pi), np.arccos(np.clip(-n[1], -1.0, 1.0)) / np.pi])


class Reanchored:
    """What compare_paths_reanchored saw: paths, bounces compared, allowed flips [(px, row, sample, bounce, what)], and per quantity the
    largest distance beyond the oracle's hull in units of eps x scale (strict: the largest relative difference)."""

    def __init__(self):
        self.paths, self.bounces, self.flips, self.excess, self.mat_map = 0, 0, [], {}, {}

    def note(self, what, x):
        self.excess[what] = max(self.excess.get(what, 0.0), float(x))

    def report(self, label=""):
        return "%s %d paths, %d bounces, %d allowed flips %s; beyond the hull (eps x scale): %s" % (
            label, self.paths, self.bounces, len(self.flips), self.flips,
            ", ".join("%s %.3g" % (k, v) for k, v in sorted(self.excess.items())))


def compare_paths_reanchored(product_probe, oracle_scene, cam, p, pairs, eps, K=8.0, w=32.0, strict_tol=None, max_flip_share=0.02,
                             n_media=2, max_out=64):
    """The product's own path, re-anchored at every bounce: record k's ray goes to the f64 oracle's world.hit() (rto_probe_hit, the
    draws of the same (seed, pixel, sample, bounce) key), the product's hit record to the oracle's Material::scatter + emitted
    (rto_probe_scatter), so rounding never accumulates along a path and every bounce is held to the product's own arithmetic.
    product_probe(px, row, sample) -> (records [n, 20], tail [4]) (product_probe_tail).  Checked per (px, row, sample):
      camera   record 0's ray == Camera::ray(s, t) of the keyed jitter (s = (px + u) / W, t = (H - 1 - row + v) / H)
      hit      hit or miss, material (the oracle's graph ids map one-to-one and order preserving onto the product's flat indices),
               front_face, t, p, normal, and (u, v) where the product computes them
      scatter  scattered or absorbed, attenuation.r, emitted.r, and record k+1's ray == the scattered ray
      end      a path that ended by a miss (fewer than max_depth and max_out records, the last one scattered): the oracle's
               continuation misses too
      radiance the probe's tail (path_step(): the steps the trace kernels run) == sum_k emitted_k prod_{j<k} att_j of the oracle's three
               channels along the product's path; the tail's bounce count == the records'
    CONTINUOUS values: the oracle is evaluated at the product's input and at its 12 one-coordinate perturbations (_ray_perturbations;
    for the scatter the direction's six and six of the hit point, +-K eps max(|p|, 1)): the product's value lies in the hull of those
    results widened by w eps scale, so the conditioning of each operation is measured, not assumed; for a sphere whose |o - centre| (or,
    under f64's textbook discriminant, |o - centre|^2 / r) dwarfs |o| and |p| the origin is also moved by K eps times that, which is
    moving the sphere.  Scales: t max(1, |t|, |o| / |d|), p and the scattered origin max(1, |o| + |t d|), a sphere's normal that / r
    (its (u, v) also take the normal moved by that budget), other normals and (u, v) 1, attenuation / emission max(1, |x|), the scattered direction
    max(1, |d'|, |p|) (the reference forms it as (p + n + ball) - p), the camera ray max(1, |o|, |d|) (lower-left corner + s horizontal
    + t vertical - origin); f32 media add what the 24 significant bits of their log draw move the free flight
    (eps max(1, t) / min_m |ln U_m|).  DECISIONS (hit or miss, which material, front_face, scattered or absorbed, the unit-ball draw's
    rejection loop, a dielectric reflecting or refracting): a product decision the oracle does not take at the product's input is an
    ALLOWED FLIP only when one of the perturbed evaluations takes it (the ball: a candidate with | |v|^2 - 1 | <= 2K eps; a dielectric:
    |u - schlick(cos)| <= K eps or |ri sin - 1| <= K eps); the path is not compared after it; flips are counted and must stay within
    `max_flip_share` of the paths.  Anything else fails.
    `strict_tol` (the IEEE-strict build): no perturbation, no flip, every value within strict_tol x scale of the oracle at the product's
    input.  Returns a Reanchored."""
    from oracle import rto
    res = Reanchored()
    mat_map, inv = res.mat_map, {}
    W, H, seed, quirks, t_min = p.width, p.height, p.seed, p.quirks, p.t_min
    strict = strict_tol is not None
    f32 = eps > 1e-10
    failures = []

    def fail(*what):
        failures.append(what)

    def mat_ok(om, pm):
        return mat_map[om] == pm if om in mat_map else pm not in inv

    def beyond(x, vals, scale, what, where):
        """How far x lies outside the hull of vals, in units of eps x scale (strict: relative to the centre value, in units of scale)."""
        x, vals = np.asarray(x, dtype=np.float64), np.asarray(vals, dtype=np.float64).reshape(-1, np.size(x))
        if strict:
            ex = np.abs(x - vals[0]).max() / scale
            res.note(what, ex)
            if not ex <= strict_tol:
                fail(what, where, x, vals[0], ex)
            return
        lo, hi = vals.min(axis=0), vals.max(axis=0)
        ex = np.maximum(np.maximum(lo - x, x - hi), 0.0).max() / (eps * scale)
        res.note(what, ex)
        if not ex <= w:
            fail(what, where, x, lo, hi, ex)

    def rays_of(ray):
        return [ray] if strict else _ray_perturbations(ray, eps, K)

    for (px, row, s) in pairs:
        recs, tail = product_probe(px, row, s)
        n = len(recs)
        pixel = row * W + px
        res.paths += 1
        u = rto.probe_uniform(seed, pixel, s, 0, rto.SLOT_JITTER_U)
        v = rto.probe_uniform(seed, pixel, s, 0, rto.SLOT_JITTER_V)
        cr = rto.probe_camera_ray(cam, (px + u) / W, (H - 1 - row + v) / H, seed, pixel, s)
        if n == 0:   # the camera ray missed everything
            hits = [rto.probe_hit(oracle_scene, r, t_min, seed, pixel, s, 0, quirks) for r in rays_of(cr)]
            if hits[0] is not None:
                if any(h is None for h in hits[1:]):
                    res.flips.append((px, row, s, 0, "miss"))
                    continue
                fail("miss", (px, row, s, 0), hits[0])
            if not (np.all(tail[0:3] == 0.0) and tail[3] == 0):
                fail("radiance of a miss", (px, row, s), tail)
            continue
        sc_cam = max(1.0, np.abs(cr[0:6]).max())
        beyond(recs[0][11:17], [cr[0:6]], sc_cam, "camera ray", (px, row, s))
        beyond(recs[0][17:18], [cr[6:7]], max(1.0, abs(cr[6])), "camera time", (px, row, s))
        L_lo, L_hi, thr_lo, thr_hi = np.zeros(3), np.zeros(3), np.ones(3), np.ones(3)
        cut = False
        for k in range(n):
            a = recs[k]
            ray = a[11:18].copy()
            where = (px, row, s, k)
            # ---- world.hit at the product's ray
            p_abs = np.abs(a[1:4]).max()
            evals = [(r, rto.probe_hit(oracle_scene, r, t_min, seed, pixel, s, k, quirks))
                     for r in ([ray] if strict else _ray_perturbations(ray, eps, K, p_abs))]
            pm, pff = int(a[7]), a[10]

            def agrees(h):
                return h is not None and h[9] == pff and mat_ok(int(h[10]), pm)
            c = evals[0][1]
            radii = []
            if not strict and agrees(c):
                # the object's own coordinates: a sphere's test rounds |o - centre| (and the f64 kernels' textbook discriminant
                # half_b^2 - a (|oc|^2 - r^2), the reference's, |oc|^2: the surface moves by eps |oc|^2 / 2r), which may be far larger than
                # |o| and |p| (random_scene's ground, r = 1000; spheres_1m's small spheres seen from afar).  Moving the object by delta is
                # moving the ray by -delta: the origin is perturbed by K eps size as well, the sphere's r = |dp| / |dn| from the oracle's
                # hits for the origin moved by 1e-6 max(|p|, 1) (a plane: dn = 0, nothing to add)
                step = 1e-6 * max(p_abs, 1.0)
                for ax in range(2):
                    r2 = ray.copy(); r2[ax] += step
                    h = rto.probe_hit(oracle_scene, r2, t_min, seed, pixel, s, k, quirks)
                    dn = np.linalg.norm(h[4:7] - c[4:7]) if agrees(h) else 0.0
                    if dn > 0.0:
                        radii.append(np.linalg.norm(h[1:4] - c[1:4]) / dn)
                if radii:
                    r_s = float(np.median(radii))
                    oc = np.abs(ray[0:3] - (c[1:4] - r_s * (c[4:7] if c[9] == 1.0 else -c[4:7]))).max()
                    size = max(oc + r_s, oc * oc / r_s if not f32 else 0.0)
                    # (at 1/4 and 1/16 of the step too: near a decision one side of the full step may take another object and leave the hull)
                    if size > 2.0 * max(p_abs, np.abs(ray[0:3]).max(), 1.0):
                        evals += [(r, rto.probe_hit(oracle_scene, r, t_min, seed, pixel, s, k, quirks))
                                  for f in (1.0, 0.25, 0.0625) for r in _ray_perturbations(ray, eps, K, f * size)[1:]]
            if not agrees(c):
                if not strict and any(agrees(h) for _, h in evals[1:]):
                    res.flips.append(where + ("hit",))
                    cut = True
                    break
                fail("hit decision", where, a[0:11], c)
                cut = True
                break
            om = int(c[10])
            if om not in mat_map:
                mat_map[om] = pm
                inv[pm] = om
            res.bounces += 1
            same = [(r, h) for r, h in evals if agrees(h)]
            hs = np.array([h for _, h in same])
            o_abs, d_abs = np.abs(ray[0:3]).max(), np.abs(ray[3:6]).max()
            sc_t = max(1.0, abs(a[0]), o_abs / max(d_abs, 1e-300))
            sc_p = max(1.0, o_abs + abs(a[0]) * d_abs)
            medium = (not strict and f32 and c[4] == 1.0 and c[5] == 0.0 and c[6] == 0.0 and c[7] == 0.0 and c[8] == 0.0
                      and a[4] == 1.0 and a[5] == 0.0 and a[6] == 0.0)
            if medium:   # the free flight's log draw: 24 significant bits of U move -ln(U) / density by eps (1 + |ln U|) / density
                lnu = min(abs(np.log(rto.probe_uniform(seed, pixel, s, k + 1, rto.SLOT_MEDIUM + m))) for m in range(n_media))
                draw = max(1.0, abs(a[0])) * (1.0 + 1.0 / max(lnu, 1e-300)) / w
                sc_t += draw
                sc_p += draw * d_abs
            beyond(a[0:1], hs[:, 0:1], sc_t, "t", where)
            # (moving the object by -delta instead of the ray by delta: the same t, normal and (u, v), the point moved by -delta)
            rs = np.array([r for r, h in same])
            beyond(a[1:4], np.concatenate([hs[:, 1:4], hs[:, 1:4] - (rs[:, 0:3] - ray[0:3])]), sc_p, "p", where)
            # a sphere's normal (p - centre) / r carries the rounding of p / r, across the surface as well (the oracle's points lie on it)
            sc_n = max(1.0, sc_p / float(np.median(radii))) if radii else 1.0
            beyond(a[4:7], hs[:, 4:7], sc_n, "normal", where)
            if a[8] != 0.0 or a[9] != 0.0:
                uvs = hs[:, 7:9]
                if radii and np.abs(_sphere_uv(c[4:7] if c[9] == 1.0 else -c[4:7]) - c[7:9]).max() <= 1e-9:
                    # a world-space sphere: its (u, v) are those of the normal, and the normal carries w eps sc_n of rounding — near a pole
                    # acos(-y) turns that into sqrt(2 w eps sc_n) / pi: the (u, v) of the product's normal moved by it belong to the hull
                    nrm = a[4:7] if a[10] == 1.0 else -a[4:7]
                    dn = w * eps * sc_n
                    uvs = np.concatenate([uvs] + [[_sphere_uv(nrm + sg * dn * np.eye(3)[i])] for i in range(3) for sg in (-1.0, 1.0)])
                beyond(a[8:10], uvs, 1.0, "uv", where)
            # ---- scatter + emitted of the product's record
            rec_in = np.array([a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[8], a[9], a[10]])
            sins = [(ray, rec_in)]
            if not strict:
                sins += [(r, rec_in) for r in _ray_perturbations(ray, eps, K)[1:] if np.any(r[3:6] != ray[3:6])]
                dp = K * eps * max(np.abs(rec_in[1:4]).max(), 1.0)
                for ax in range(3):
                    for sg in (-1.0, 1.0):
                        rr = rec_in.copy(); rr[1 + ax] += sg * dp; sins.append((ray, rr))
            outs = np.array([rto.probe_scatter(oracle_scene, om, r, rr, seed, pixel, s, k) for r, rr in sins])
            scattered = a[19] >= 0.0
            if (outs[0, 0] == 1.0) != scattered:
                if not strict and np.any((outs[1:, 0] == 1.0) == scattered):
                    res.flips.append(where + ("absorbed",))
                    cut = True
                    break
                fail("scattered", where, a[18:20], outs[0])
                cut = True
                break
            sel = outs[(outs[:, 0] == 1.0) == scattered]
            beyond(a[18:19], sel[:, 10:11], max(1.0, abs(a[18])), "emitted", where)
            tol_c = strict_tol if strict else w * eps
            e_lo, e_hi = sel[:, 10:13].min(axis=0), sel[:, 10:13].max(axis=0)
            e_lo, e_hi = e_lo - tol_c * np.maximum(1.0, np.abs(e_lo)), e_hi + tol_c * np.maximum(1.0, np.abs(e_hi))
            L_lo += thr_lo * np.maximum(e_lo, 0.0)
            L_hi += thr_hi * e_hi
            if not scattered:
                break
            beyond(a[19:20], sel[:, 1:2], max(1.0, abs(a[19])), "attenuation", where)
            a_lo, a_hi = sel[:, 1:4].min(axis=0), sel[:, 1:4].max(axis=0)
            thr_lo = thr_lo * np.maximum(a_lo - tol_c * np.maximum(1.0, np.abs(a_lo)), 0.0)
            thr_hi = thr_hi * (a_hi + tol_c * np.maximum(1.0, np.abs(a_hi)))
            if k + 1 < n:
                b = recs[k + 1]
                beyond(b[11:14], sel[:, 4:7], sc_p, "scattered origin", where)
                if b[17] != a[17]:
                    fail("ray time", where, a[17], b[17])
                nf = len(failures)
                sc_d = max(1.0, np.abs(b[14:17]).max(), np.abs(a[1:4]).max())
                beyond(b[14:17], sel[:, 7:10], sc_d, "scattered direction", where)
                if len(failures) > nf and not strict:   # the direction is another one: a rounding-decided draw or branch?
                    c0 = outs[0]
                    ball = _ball_is_ambiguous(seed, pixel, s, k, 2.0 * K * eps)
                    diel = False
                    if np.all(c0[1:4] == 1.0) and c0[0] == 1.0:   # a dielectric (the only material with a white attenuation here)
                        nrm = a[4:7]
                        ud = ray[3:6] / np.linalg.norm(ray[3:6])
                        refl = ud - 2.0 * (ud @ nrm) * nrm
                        other = b[14:17] if np.linalg.norm(b[14:17] - refl) > np.linalg.norm(c0[7:10] - refl) else c0[7:10]
                        tang_u, tang_o = ud - (ud @ nrm) * nrm, other - (other @ nrm) * nrm
                        ratio = np.linalg.norm(tang_o) / max(np.linalg.norm(tang_u), 1e-300)
                        cos_t = min(-(ud @ nrm), 1.0)
                        sin_t = np.sqrt(max(1.0 - cos_t * cos_t, 0.0))
                        uu = rto.probe_uniform(seed, pixel, s, k + 1, rto.SLOT_DIELECTRIC)
                        diel = (abs(uu - rto.probe_schlick(cos_t, ratio)) <= K * eps or abs(ratio * sin_t - 1.0) <= K * eps)
                    if ball or diel:
                        del failures[nf:]
                        res.flips.append(where + ("ball" if ball else "dielectric",))
                        cut = True
                        break
            elif n < p.max_depth and n < max_out:   # the product's continuation missed: so must the oracle's
                cont = np.concatenate([outs[0, 4:10], a[17:18]])
                hits = [rto.probe_hit(oracle_scene, r, t_min, seed, pixel, s, k + 1, quirks) for r in rays_of(cont)]
                if hits[0] is not None:
                    if not strict and any(h is None for h in hits[1:]):
                        res.flips.append(where + ("end",))
                        cut = True
                        break
                    fail("end of path", where, hits[0])
        if cut:
            continue
        # ---- the tail: path_step()'s radiance along the same path, and its bounce count
        expect_bounces = n - 1 if recs[n - 1][19] < 0.0 else n
        if tail[3] != expect_bounces:
            fail("tail bounces", (px, row, s), tail[3], expect_bounces)
        unit_L = (1.0 if strict else eps) * np.maximum(1.0, L_hi)
        exL = (np.maximum(np.maximum(L_lo - tail[0:3], tail[0:3] - L_hi), 0.0) / unit_L).max()
        res.note("radiance", exL)
        if not exL <= (strict_tol if strict else w + n):   # (+ n: the product's throughput is a product of n rounded factors)
            fail("radiance", (px, row, s), tail[0:3], L_lo, L_hi)
    ids = sorted(mat_map)
    flat = [mat_map[i] for i in ids]
    if flat != sorted(flat):
        fail("material order", mat_map)
    if len(res.flips) > max_flip_share * max(res.paths, 1):
        fail("flips", len(res.flips), res.paths, res.flips)
    print(res.report())
    assert not failures, (len(failures), failures[:6], res.report())
    return res


# ---- node records (include/rttnw_hip.h rttnw_debug_scene_nodes / rttnw_debug_scene_nodes4)
NODE2 = np.dtype([("lo0", "<f4", 3), ("hi0", "<f4", 3), ("lo1", "<f4", 3), ("hi1", "<f4", 3), ("child", "<i4", 2), ("pad", "<i4", 2)])
NODE4 = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("child", "<i4", 4), ("pad", "<i4", 4)])
assert NODE2.itemsize == 64 and NODE4.itemsize == 128
CHILD_EMPTY = -2**31


def nodes_of(binding, sc, wide=False):
    fn = binding.debug_scene_nodes4 if wide else binding.debug_scene_nodes
    n = fn(sc.handle, None, 0, None)
    buf = np.zeros(n, dtype=NODE4 if wide else NODE2)
    root = C.c_int32()
    assert fn(sc.handle, buf.ctypes.data, n, C.byref(root)) == n
    return buf, root.value


def leaves_of_binary(nodes, root):
    out, stack = [], [root]
    while stack:
        nd = nodes[stack.pop()]
        for ch in nd["child"]:
            if ch >= 0:
                stack.append(int(ch))
            elif ch != CHILD_EMPTY:
                out.append(int(ch))
    return sorted(out)


def check_wide_tree(nodes4, root):
    """Walk a 4-wide tree: every record reached once, a child's boxes inside the slot box its parent holds for it, unused
    slots empty.  Returns (sorted leaf codes, stack entries a walk can have pending = what the lowering must bound)."""
    leaves, seen = [], set()

    def visit(i, plo, phi):
        assert i not in seen
        seen.add(i)
        nd = nodes4[i]
        k, deepest = 0, 0
        for c in range(4):
            ch, lo, hi = int(nd["child"][c]), nd["lo"][:, c], nd["hi"][:, c]
            if ch == CHILD_EMPTY:
                assert (lo > hi).all()
                continue
            k += 1
            assert (lo <= hi).all() and (lo >= plo).all() and (hi <= phi).all()
            if ch >= 0:
                deepest = max(deepest, visit(ch, lo, hi))
            else:
                leaves.append(ch)
        return max(k - 1, 0) + deepest

    need = visit(root, np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32))
    return sorted(leaves), need, seen
