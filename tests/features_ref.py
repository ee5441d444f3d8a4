"""TEST INFRASTRUCTURE for rttnw_render_features: the expected feature buffers composed, sample by sample, from the CPU oracle's own
operations — rto.probe_uniform (the jitter) -> rto.probe_camera_ray -> rto.probe_hit (bounce 0) -> rto.probe_scatter — summed in sample
order, as the contract in include/rttnw_hip.h states them."""
import numpy as np

from oracle import rto


def sample_features(oracle_scene, cam, p, px, row, sample, perturb=0.0):
    """(albedo[3], normal[3], depth, alpha, decision) of one sample of one pixel; `decision` = (material, front_face, scattered) or None
    for a miss.  perturb > 0: also the decisions for the camera ray moved by that much (relative) in each coordinate -> a set."""
    W, H, seed = p.width, p.height, p.seed
    pixel = row * W + px
    u = rto.probe_uniform(seed, pixel, sample, 0, rto.SLOT_JITTER_U)
    v = rto.probe_uniform(seed, pixel, sample, 0, rto.SLOT_JITTER_V)
    cr = rto.probe_camera_ray(cam, (px + u) / W, (H - 1 - row + v) / H, seed, pixel, sample)

    def at(ray):
        hit = rto.probe_hit(oracle_scene, ray, p.t_min, seed, pixel, sample, 0, p.quirks)
        if hit is None:
            return np.array(p.background[:]), np.zeros(3), 0.0, 0.0, None
        rec = np.array([hit[0], hit[1], hit[2], hit[3], hit[4], hit[5], hit[6], hit[7], hit[8], hit[9]])
        out = rto.probe_scatter(oracle_scene, int(hit[10]), ray, rec, seed, pixel, sample, 0)
        scattered = out[0] == 1.0
        d = ray[3:6]
        depth = hit[0] * np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        return (out[1:4] if scattered else out[10:13]).copy(), hit[4:7].copy(), depth, 1.0, (int(hit[10]), hit[9], scattered)

    albedo, normal, depth, alpha, decision = at(cr)
    if perturb <= 0.0:
        return albedo, normal, depth, alpha, decision
    decisions = {decision}
    do = perturb * max(np.abs(cr[0:3]).max(), 1.0)
    dd = perturb * np.abs(cr[3:6]).max()
    for a in range(3):
        for sg in (-1.0, 1.0):
            r = cr.copy(); r[a] += sg * do; decisions.add(at(r)[4])
            r = cr.copy(); r[3 + a] += sg * dd; decisions.add(at(r)[4])
    return albedo, normal, depth, alpha, decisions


def expected(oracle_scene, cam, p, perturb=0.0):
    """The frame's features: {"albedo": HxWx3, "normal": HxWx3, "depth": HxW, "alpha": HxW}, each channel one chain in sample order then
    one division by spp — and, with perturb > 0, the HxW mask of pixels one of whose samples changes its first-hit decision under it."""
    H, W = p.height, p.width
    out = {"albedo": np.zeros((H, W, 3)), "normal": np.zeros((H, W, 3)), "depth": np.zeros((H, W)), "alpha": np.zeros((H, W))}
    fragile = np.zeros((H, W), dtype=bool)
    for row in range(H):
        for px in range(W):
            a, n, z, c = np.zeros(3), np.zeros(3), 0.0, 0.0
            for s in range(p.spp):
                sa, sn, sz, sc, dec = sample_features(oracle_scene, cam, p, px, row, p.sample_begin + s, perturb)
                a, n, z, c = a + sa, n + sn, z + sz, c + sc
                if perturb > 0.0 and len(dec) > 1:
                    fragile[row, px] = True
            out["albedo"][row, px], out["normal"][row, px], out["depth"][row, px], out["alpha"][row, px] = a / p.spp, n / p.spp, z / p.spp, c / p.spp
    return (out, fragile) if perturb > 0.0 else out


def deviation(got, want):
    """Per pixel, the largest channel difference relative to max(1, |value|) over albedo, normal, depth and alpha."""
    d = np.zeros(want["alpha"].shape)
    for k in ("albedo", "normal", "depth", "alpha"):
        e = np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
        d = np.maximum(d, e.max(axis=2) if e.ndim == 3 else e)
    return d
