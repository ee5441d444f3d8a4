// scene_narrow.hpp — from the lowering's f64 master copy (scene_lower.hpp FlatScene) to the records, arrays and camera of ONE precision R.
// The only place a record is narrowed: the device upload (render_common.hpp DeviceScene) and the host build of the core (tests/hostsim)
// both go through it, so what the CPU suite walks is what the kernels are handed.  Pure C++; no HIP in here.
#pragma once
#include "../../include/rttnw_hip.h"
#include "rt_types.hpp"
#include "scene_lower.hpp"

#include <vector>

namespace rt {

// narrow<R>(record): every real field cast to R, every integer copied.  One brace initialiser in declaration order wherever the record allows
// it: a member added to a record and forgotten here is then a -Wextra warning of the host build (missing initialiser), not a silent zero.
#define RT_NARROW3(a) {R((a)[0]), R((a)[1]), R((a)[2])}
template <typename R> SphereRec<R> narrow(const SphereRec<double>& s) { return {R(s.cx), R(s.cy), R(s.cz), R(s.r)}; }
template <typename R> MovingSphereRec<R> narrow(const MovingSphereRec<double>& m) {
    return {RT_NARROW3(m.c0), R(m.r), RT_NARROW3(m.c1), R(m.t0), R(m.t1), m.mat, m.seq};
}
template <typename R> RectRec<R> narrow(const RectRec<double>& r) { return {R(r.a0), R(r.a1), R(r.b0), R(r.b1), R(r.k), r.plane, r.mat, r.seq}; }
template <typename R> BoxRec<R> narrow(const BoxRec<double>& b) { return {RT_NARROW3(b.mn), RT_NARROW3(b.mx), b.mat, b.seq}; }
template <typename R> InstanceRec<R> narrow(const InstanceRec<double>& i) {
    InstanceRec<R> o{}; // (an array of ops: filled in a loop, pads 0)
    o.n_ops = i.n_ops; o.root = i.root; o.single_leaf = i.single_leaf;
    for (int k = 0; k < MAX_INSTANCE_OPS; ++k) {
        o.ops[k].type = i.ops[k].type;
        for (int c = 0; c < 3; ++c) o.ops[k].v[c] = R(i.ops[k].v[c]);
    }
    return o;
}
template <typename R> MediumRec<R> narrow(const MediumRec<double>& m) {
    return {m.b_first, m.b_count, m.inst, m.n_outer, m.mat, m.ref0, R(m.neg_inv_density)};
}
template <typename R> MaterialRec<R> narrow(const MaterialRec<double>& m) { return {m.type, m.tex, RT_NARROW3(m.albedo), R(m.param)}; }
template <typename R> TextureRec<R> narrow(const TextureRec<double>& t) { return {t.type, t.a, t.b, 0, RT_NARROW3(t.color), R(t.scale)}; }
template <typename R> CameraRec<R> narrow(const CameraRec<double>& c) {
    return {RT_NARROW3(c.origin), RT_NARROW3(c.lower_left_corner), RT_NARROW3(c.horizontal), RT_NARROW3(c.vertical), RT_NARROW3(c.u), RT_NARROW3(c.v),
            R(c.lens_radius), R(c.open_time), R(c.close_time)};
}
#undef RT_NARROW3

// A lowered scene's real-valued arrays in precision R, in host memory.  The integer arrays (nodes, sphere_mat, sphere_seq, medium_refs, images,
// texels, perlin_perm) have one form for every precision and stay in the FlatScene.
template <typename R> struct NarrowScene {
    std::vector<SphereRec<R>> spheres;
    std::vector<MovingSphereRec<R>> moving;
    std::vector<RectRec<R>> rects;
    std::vector<BoxRec<R>> boxes;
    std::vector<InstanceRec<R>> insts;
    std::vector<MediumRec<R>> media;
    std::vector<MaterialRec<R>> mats;
    std::vector<TextureRec<R>> texs;
    std::vector<R> perlin_vec;

    explicit NarrowScene(const FlatScene& f) {
        all(spheres, f.spheres); all(moving, f.moving); all(rects, f.rects); all(boxes, f.boxes); all(insts, f.insts); all(media, f.media);
        all(mats, f.mats); all(texs, f.texs);
        perlin_vec.reserve(f.perlin_vec.size());
        for (double v : f.perlin_vec) perlin_vec.push_back(R(v));
    }
    // The scene as code that runs on the host walks it: these vectors and f's integer arrays, by pointer (the host-built node records; no
    // quantised ones).  `f` and this object must outlive the view.
    void fill_view(const FlatScene& f, SceneView<R>& v) const {
        v.nodes = f.nodes4.data(); v.nodes4q = nullptr;
        v.spheres = spheres.data(); v.sphere_mat = f.sphere_mat_is_index ? nullptr : f.sphere_mat.data(); v.sphere_seq = f.sphere_seq.data();
        v.moving = moving.data(); v.rects = rects.data(); v.boxes = boxes.data(); v.insts = insts.data(); v.media = media.data();
        v.medium_refs = f.medium_refs.data(); v.mats = mats.data(); v.texs = texs.data(); v.images = f.images.data(); v.texels = f.texels.data();
        v.perlin_vec = perlin_vec.data(); v.perlin_perm = f.perlin_perm.data();
        v.top_root = f.top_root; v.n_media = int32_t(media.size());
    }

  private:
    template <typename Out, typename In> static void all(Out& out, const In& in) {
        out.reserve(in.size());
        for (const auto& rec : in) out.push_back(narrow<R>(rec));
    }
};

// The camera of a render in precision R: Camera::new in f64 on the host (scene_lower.cpp make_camera), then narrowed.
template <typename R> CameraRec<R> camera_of(const rttnw_camera_desc* cam) {
    CameraRec<double> c;
    make_camera(cam->lookfrom, cam->lookat, cam->view_up, cam->vertical_fov, cam->aspect_ratio, cam->aperture, cam->focus_distance, cam->open_time,
                cam->close_time, c);
    return narrow<R>(c);
}

} // namespace rt
