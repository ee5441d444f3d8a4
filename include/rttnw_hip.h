/*
 * rttnw_hip.h — C ABI of the MI355X-native path tracer that drops in behind
 * luliic2/rttnw's `scenes.rs` / `main.rs::render`.
 *
 * The reference has no FFI; the seam that exists is the Rust-level surface between
 * `src/scenes.rs` + `src/main.rs` (callers) and `src/math/` (the tracing core).  Every entry
 * point below replaces one constructor / method of that surface; the reference item is cited
 * next to it as `file:line` relative to the reference repo root.  `dyn Hittable` objects expose
 * only `hit`/`bounding_box`, so they cannot be lowered after the fact: a host describes the scene
 * through these calls instead of (or next to) building trait objects.  INTEGRATION.md shows the
 * Rust `extern "C"` block and the `scenes.rs`-shaped wrapper a maintainer would add.
 *
 * Conventions
 *   - plain C, POD only, no callbacks; doubles on the boundary (the reference is f64 throughout,
 *     src/math/vec3.rs:12); the library narrows to f32 itself when `precision == RTTNW_F32`.
 *   - objects (textures, materials, hittables) are `rttnw_id` handles owned by their scene; a
 *     negative id is an error code.  Handles may be shared (Arc semantics, e.g. one material on
 *     many spheres, scenes.rs:317-324).
 *   - functions returning `int` return RTTNW_OK (0) or a negative RTTNW_ERR_*;
 *     `rttnw_last_error()` returns a thread-local message for the last failure.
 *   - a scene is mutable until `rttnw_scene_commit`, immutable afterwards (the reference shares
 *     `&world` immutably across rayon workers, main.rs:216); one render in flight per scene.
 *     One exception, inside the library: the trees are built for the shutter interval [0, 1]
 *     (`BvhTree::from`, hittable.rs:256); the first render whose camera shutter reaches outside
 *     it rebuilds them for the wider interval (`BvhTree::from_time`, hittable.rs:261) before it
 *     enqueues anything — under a lock, device copies re-uploaded on use, and
 *     `rttnw_scene_build_info` reports the rebuilt trees from then on.
 *   - there is NO CPU fallback: every render entry point fails with RTTNW_ERR_HIP when no gfx950
 *     device is usable.
 */
#ifndef RTTNW_HIP_H
#define RTTNW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTTNW_ABI_VERSION 3 /* 2: 4-wide node records (n_nodes, debug_scene_nodes4), rttnw_render_multi
                             * 3: RTTNW_F64_STRICT, rttnw_shutdown, RTTNW_BVH_AUTO (the default builder), rttnw_stats.reserved is a bit mask
                             *    (below), validate() rejects t_min < 0
                             * (rttnw_render_adaptive, rttnw_render_features / rttnw_denoise, rttnw_render_region, rttnw_render_adaptive_multi,
                             *  rttnw_render_adaptive_resume with rttnw_adaptive_state_doubles, rttnw_render_adaptive_region,
                             *  rttnw_render_adaptive_denoised, rttnw_reconstruct, rttnw_render_preview, rttnw_budget_select,
                             *  rttnw_render_adaptive_budget, rttnw_render_adaptive_budget_denoised, rttnw_denoise_nlm,
                             *  rttnw_denoise_select, rttnw_temporal_accumulate, rttnw_temporal_variance, the rttnw_svgf_create family, rttnw_temporal_clamp,
                             *  rttnw_svgf_set_clamp, rttnw_svgf_clipped, rttnw_temporal_probe, rttnw_svgf_set_sampling, rttnw_svgf_samples,
                             *  rttnw_denoise_regress, rttnw_svgf_set_regress, rttnw_svgf_push_halves and rttnw_svgf_halves came later, without a version bump: a caller detects each by its symbol) */

typedef struct rttnw_scene rttnw_scene; /* opaque */
typedef int32_t rttnw_id;

enum rttnw_status {
    RTTNW_OK = 0,
    RTTNW_ERR_INVALID = -1,     /* bad argument / unknown id / wrong object kind */
    RTTNW_ERR_STATE = -2,       /* call not allowed in this scene state (e.g. edit after commit) */
    RTTNW_ERR_UNSUPPORTED = -3, /* scene graph shape the lowering does not handle */
    RTTNW_ERR_HIP = -4,         /* HIP runtime error or no usable device */
    RTTNW_ERR_NOMEM = -5
};

/* Plane selector of `Rectangle<M,P>`: (axis0, axis1, k) — hittable.rs:450-488. */
enum rttnw_plane { RTTNW_XY = 0, RTTNW_XZ = 1, RTTNW_YZ = 2 };

/* Arithmetic type of the render kernels.
 *   RTTNW_F64  the reference's type (vec3.rs:12) and the PARITY mode: images equal the f64 restatement of the reference
 *              to <= 1e-9 per channel (RGBA8 identical at 800x800 spp 1000), every bounce's hit record to 1e-9.
 *   RTTNW_F32  a THROUGHPUT mode (about 1.5x the rate), NOT a peer precision: equal seeds share every random decision
 *              with f64 up to rounding, the estimator is unbiased (every pixel within 6 sigma / sqrt(spp) + 1/256 of
 *              the f64 image, crop means within 0.5 %), but on scenes with small specular / refractive / fuzzy spheres
 *              (final_scene: the r = 10 cluster, glass, fuzz-1 metal) an f32 path and its f64 twin diverge after a few
 *              bounces, so RGBA8 agrees within 1 LSB on 96.7 % of the pixels at spp 1000 there (cornell_box: 99 %) —
 *              outside the >= 99 % of the parity tier (tests/test_gpu_parity.py::test_T2_at_baseline_size).
 *   RTTNW_F64_STRICT  f64 with NOTHING contracted and every quotient an IEEE division — the operations of the reference's Rust in
 *              its order (rustc fuses no multiply-add): every path takes the decisions of the CPU reference bit for bit, where
 *              RTTNW_F64 (built with fused multiply-adds and shared reciprocals) agrees to rounding only — which a scene that
 *              amplifies rounding (config 5: a million small spheres, ~100x per bounce) turns into different paths after a few
 *              bounces.  It also tests every object in the frame the reference tests it in: a scene whose default lowering holds
 *              world-space copies of transformed groups' spheres is lowered a second time at its first strict render — the copies'
 *              world-space BOXES stay in the top tree (culling never shapes a result), the sphere test itself is made through the
 *              group's wrappers as in hittable.rs:599-606,686-699 (final_scene: every pixel within 1e-12 of the CPU reference at
 *              800x800 spp 5000, RGBA8 identical).  Same buffers as RTTNW_F64 (doubles); 5-10 % slower on cornell_box, 15-18 % on
 *              final_scene (what it costs, measured: IEEE quotients 6 %, no contraction 3 %, registers the rest), nothing on config 5. */
enum rttnw_precision { RTTNW_F64 = 0, RTTNW_F32 = 1, RTTNW_F64_STRICT = 2 };

/* Bit flags for `rttnw_params.quirks`. */
#define RTTNW_QUIRK_YROTATE_BACKROT 1u /* Q1: hittable.rs:700-705 reuses the overwritten x */
#define RTTNW_QUIRKS_REFERENCE RTTNW_QUIRK_YROTATE_BACKROT

/* ---------------------------------------------------------------- lifecycle ---------------- */

/* `scene_seed` feeds the library-side scene randomness the reference draws from `thread_rng()`
 * while constructing objects: Perlin tables (noise.rs:15-29,40-47).  Generator spec: DESIGN.md. */
int rttnw_scene_create(uint64_t scene_seed, rttnw_scene** out);
void rttnw_scene_destroy(rttnw_scene* scene);

/* ---------------------------------------------------------------- textures (texture.rs) ---- */

/* `impl Texture for Vec3f<Color>` — texture.rs:9-13 */
rttnw_id rttnw_tex_solid(rttnw_scene* s, double r, double g, double b);
/* `CheckerTexture { odd, even }` — texture.rs:15-30 */
rttnw_id rttnw_tex_checker(rttnw_scene* s, rttnw_id odd, rttnw_id even);
/* `NoiseTexture::scaled(scale)` (owns a fresh `Perlin::new()`) — texture.rs:45-59, noise.rs:40-47 */
rttnw_id rttnw_tex_noise(rttnw_scene* s, double scale);
/* `ImageTexture::new(path)` — texture.rs:64-107.  The host decodes the file; the library copies
 * `w*h*4` bytes (RGBA8, row-major, top row first; alpha ignored).  `rgba == NULL` reproduces the
 * load-failure behaviour: constant cyan (texture.rs:102-105). */
rttnw_id rttnw_tex_image_rgba8(rttnw_scene* s, const uint8_t* rgba, uint32_t w, uint32_t h);

/* ---------------------------------------------------------------- materials (material.rs) -- */

/* `Lambertian::arc/boxed(texture_or_colour)` — material.rs:25-100 */
rttnw_id rttnw_mat_lambertian(rttnw_scene* s, rttnw_id tex);
/* `Metal::arc(albedo, fuzz)`; fuzz is clamped to <= 1 like material.rs:114,122,129 — :103-149 */
rttnw_id rttnw_mat_metal(rttnw_scene* s, double r, double g, double b, double fuzz);
/* `Dielectric::arc(refraction_index)` — material.rs:152-204 */
rttnw_id rttnw_mat_dielectric(rttnw_scene* s, double refraction_index);
/* `DiffuseLight::arc(texture)` — material.rs:206-250 */
rttnw_id rttnw_mat_diffuse_light(rttnw_scene* s, rttnw_id tex);
/* `Isotropic { albedo }` — material.rs:252-266 (also created implicitly by constant_medium) */
rttnw_id rttnw_mat_isotropic(rttnw_scene* s, rttnw_id tex);

/* ---------------------------------------------------------------- hittables (hittable.rs) -- */

/* `Sphere { center, radius, material }` — hittable.rs:69-131 */
rttnw_id rttnw_sphere(rttnw_scene* s, const double center[3], double radius, rttnw_id mat);
/* `MovingSphere { center: c0..c1, time: t0..t1, radius, material }` — hittable.rs:179-245 */
rttnw_id rttnw_moving_sphere(rttnw_scene* s, const double center0[3], const double center1[3],
                             double time0, double time1, double radius, rttnw_id mat);
/* `XY|XZ|YZ::rectangle(material, a0..a1, b0..b1, k)` — hittable.rs:401-411,434-547 */
rttnw_id rttnw_rectangle(rttnw_scene* s, int plane, double a0, double a1, double b0, double b1,
                         double k, rttnw_id mat);
/* `Cube::new(box_min, box_max, material)` (six rectangles in a List) — hittable.rs:549-592 */
rttnw_id rttnw_cube(rttnw_scene* s, const double box_min[3], const double box_max[3], rttnw_id mat);
/* `List::new()` / `List::push(item)` — hittable.rs:134-177 */
rttnw_id rttnw_list(rttnw_scene* s);
int rttnw_list_push(rttnw_scene* s, rttnw_id list, rttnw_id item);
/* `BvhTree::from(list)` — hittable.rs:248-373.  Closest-hit results do not depend on the tree's
 * topology, so this is a grouping hint: the library builds its own flat BVH. */
rttnw_id rttnw_bvh_tree(rttnw_scene* s, rttnw_id list);
/* `Hittable::translate(offset)` — hittable.rs:51-59,594-629 */
rttnw_id rttnw_translate(rttnw_scene* s, rttnw_id item, const double offset[3]);
/* `Hittable::rotate_y(angle_degrees)` — hittable.rs:60-65,631-722 */
rttnw_id rttnw_rotate_y(rttnw_scene* s, rttnw_id item, double angle_degrees);
/* `ConstantMedium::new(boundary, density, phase_texture)` — hittable.rs:724-801 */
rttnw_id rttnw_constant_medium(rttnw_scene* s, rttnw_id boundary, double density, rttnw_id tex);

/* `Hittable::bounding_box(initial_time, final_time) -> Option<Bound>` — hittable.rs:50, the trait's second method, for any hittable id of the
 * scene's graph (before or after commit): Sphere :125-130, List :165-176, MovingSphere :233-244, BvhTree :370-372 (the bound stored by
 * `BvhTree::from` = over times 0..1, whatever is asked), Rectangle :532-546 (k -+ 0.0001), Cube :585-591, Translate :619-628, YRotate :719-721
 * (the item's box over 0..1, turned about y), ConstantMedium :798-800.  Returns 1 and writes min.xyz, max.xyz to out_min_max — 0 for `None`
 * (an empty List, a List with a member that has none) — or a negative rttnw_status.  One deliberate difference: YRotate's box is the CORRECT
 * rotation of the item's eight corners; the reference's (:661-662) rotates z with the x it has just overwritten (latent there:
 * no scene puts a YRotate into a BvhTree) and can fail to contain the object.  Nothing on the render path reads these boxes: the lowering builds
 * its own f32 boxes, rounded outward (scene_lower.cpp). */
int rttnw_hittable_bounds(const rttnw_scene* s, rttnw_id hittable, double initial_time, double final_time, double out_min_max[6]);

/* The `world: List` handed to `color()` — main.rs:47-55,216. */
int rttnw_scene_set_world(rttnw_scene* s, rttnw_id world_list);
/* Which builder `rttnw_scene_commit` uses for the flat BVHs (before commit; default RTTNW_BVH_AUTO).  Replaces the
 * reference's BvhTree::from / build (hittable.rs:300-353: recursive, random axis per level, full sort per level).
 *   RTTNW_BVH_AUTO         (ABI 3, the default) per tree: the host build below RTTNW_BVH_AUTO_DEVICE_LEAVES leaves — small trees are
 *                          tuned for the LDS-resident kernels (leaf size by what still fits) and build in well under a millisecond —,
 *                          the device binned-SAH build from there on (10^6 leaves: commit 43 instead of 165 ms at the same traversal speed)
 *   RTTNW_BVH_HOST_SAH     binned surface-area-heuristic build on the host (parallel): best traversal, 0.1 s for 10^6 leaves (commit 165 ms)
 *   RTTNW_BVH_DEVICE_LBVH  linear BVH built by HIP kernels (Morton order, Karras hierarchy, bottom-up fit):
 *                          1.4 ms for 10^6 leaves (commit 35 ms), 4-7 % slower traversal; needs a device at commit (no CPU fallback)
 *   RTTNW_BVH_DEVICE_SAH   the binned-SAH build as level-synchronous HIP kernels (binned planes for segments of more than 64
 *                          leaves, an exact sweep by one wave for smaller ones): the host builder's traversal speed at a
 *                          tenth of its build time (8.5 ms for 10^6 leaves, commit 43 ms); needs a device at commit
 * Images do not depend on the choice: the closest hit is topology independent and exact ties are resolved by
 * list order (tests/test_gpu_lbvh.py). */
#define RTTNW_BVH_HOST_SAH 0u
#define RTTNW_BVH_DEVICE_LBVH 1u
#define RTTNW_BVH_DEVICE_SAH 2u
#define RTTNW_BVH_AUTO 3u
#define RTTNW_BVH_AUTO_DEVICE_LEAVES 100000u
int rttnw_scene_set_bvh_builder(rttnw_scene* s, uint32_t builder);
/* Flatten the graph, build the flat BVHs, upload to the current HIP device.  Idempotent. */
int rttnw_scene_commit(rttnw_scene* s);

/* ---------------------------------------------------------------- render (main.rs, camera.rs) */

/* `CameraDescriptor` — camera.rs:5-15 (15 doubles, same field order). */
typedef struct rttnw_camera_desc {
    double lookfrom[3];
    double lookat[3];
    double view_up[3];
    double vertical_fov; /* degrees */
    double aspect_ratio;
    double aperture;
    double focus_distance;
    double open_time;
    double close_time;
} rttnw_camera_desc;

/* What `render()` hard-codes or takes as arguments — main.rs:58,184-197,216,33. */
typedef struct rttnw_params {
    uint32_t width;
    uint32_t height;
    uint32_t spp;        /* `samples` — main.rs:211 */
    uint32_t max_depth;  /* 50 — main.rs:216 */
    double t_min;        /* 0.001 — main.rs:33 */
    double background[3];/* main.rs:43 */
    uint64_t seed;       /* render seed of the keyed sample RNG (DESIGN.md "RNG") */
    uint32_t precision;  /* enum rttnw_precision */
    uint32_t quirks;     /* RTTNW_QUIRK_* bits; RTTNW_QUIRKS_REFERENCE reproduces the reference */
    uint32_t spp_chunk;  /* samples folded sequentially per work item; 0 = library default (4-sample chunks, the last
                            ~1/32 of the samples as single-sample chunks so that a render ends on short items).  The
                            per-pixel sum is ONE chain of chunk sums added in chunk order — a function of spp and
                            spp_chunk alone: not of the image size, the number of GPUs, or how the library splits a
                            long render into launches to keep its chunk-sum workspace within a twelfth of the GPU's memory
                            (4 .. 24 GiB; RTTNW_CHUNK_SUM_BUDGET=<bytes> overrides). */
    uint32_t tile_rank;  /* this GPU's rank in the tile partition (0 for a single GPU) */
    uint32_t tile_world; /* number of GPUs sharing the framebuffer (>= 1) */
    uint32_t collect_counters; /* 1: run the counting kernel variant and fill rttnw_stats (2: plus per-record-kind timing, 3: plus walk-length histograms; debugging) */
    uint32_t sample_begin; /* index of the first sample: this render covers samples [sample_begin, sample_begin + spp) of
                              every pixel and returns THEIR mean.  Draws are keyed by (pixel, sample), so passes over
                              disjoint ranges are independent estimates whose weighted mean is the single render of the
                              union — progressive display, checkpointed long renders (main.rs has only a progress bar). */
    uint32_t reserved0;
} rttnw_params;

typedef struct rttnw_stats {
    uint64_t samples;        /* camera paths traced by this call */
    uint64_t rays;           /* world.hit() calls (main.rs:33) */
    uint64_t nodes_visited;  /* BVH node records read */
    uint64_t prims_tested;   /* primitive records read (incl. medium boundaries) */
    uint64_t texel_fetches;  /* image-texture texel reads */
    double kernel_ms;        /* device time of the trace kernel(s), hipEvent-measured */
    uint32_t n_nodes;        /* flat scene size: 4-wide node records */
    uint32_t n_prims;
    uint32_t scene_bytes;    /* bytes of node+primitive arrays resident on the device */
    uint32_t reserved;       /* render: kernel form that ran — bit 0: decoupled (else lane-owns-path), bit 1: node records resident in LDS, bit 2: three node steps per walk trip (tiny top trees), bit 3: the instantiation whose walk never changes frames (no Translate / YRotate group with a tree of its own), bit 4: ... but tests single wrapped records in place, bit 5: ... in the LEAN flavour (the scene has no MovingSphere, no ConstantMedium and only solid colours: their code is compiled out); bit 6: the decoupled kernel walked the interleaved node + sphere buffer of a big cloud; rttnw_render_multi, rank 0 only — bit 8: the gather went through peer copies (RTTNW_MULTI_GATHER=peer), bit 9: ... because the RCCL set-up failed; rttnw_render_adaptive_budget — bits 16 .. 31: the rounds it ran (saturating): a caller that compares kernel forms across entry points masks with 0xFFFF first; scene_info: stack depth */
} rttnw_stats;

/* Framebuffer partition: 8x8-pixel tiles, tile t owned by rank
 * `rttnw_tile_owner(t) = permuted(t) % world`; each rank stores its tiles contiguously
 * ("packed" order, 64 pixels per tile, row-major inside the tile), padded to
 * `tiles_per_rank` tiles so a flat gather has a uniform count. */
typedef struct rttnw_tile_layout {
    uint32_t tiles_x, tiles_y, n_tiles;
    uint32_t tiles_per_rank; /* ceil(n_tiles / world) */
    uint32_t pixels_per_rank;/* tiles_per_rank * 64 */
} rttnw_tile_layout;
int rttnw_tile_layout_get(uint32_t width, uint32_t height, uint32_t world, rttnw_tile_layout* out);

/* `render()` for one GPU: host outputs, blocking.  Row-major, TOP ROW FIRST like main.rs:202-205.
 * `out_linear_rgb` (optional): width*height*3 doubles, the per-pixel mean radiance before gamma
 * (main.rs:217).  `out_rgba8` (optional): width*height*4 bytes after sqrt/clamp/quantise
 * (main.rs:219-225).  Requires tile_world == 1. */
int rttnw_render(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p,
                 double* out_linear_rgb, uint8_t* out_rgba8, rttnw_stats* stats);

/* Adaptive sampling: `render()` for one GPU that stops sampling a pixel once its mean is known well enough.
 *
 * Samples.  Pixel q gets samples [sample_begin, sample_begin + n_q) with n_q a multiple of B = a->pass_spp and n_q <= p->spp (the cap).
 *   Pass k traces samples [sample_begin + kB, sample_begin + (k+1)B) of every pixel still active, with the chunk schedule of a render
 *   with spp = B and the caller's spp_chunk: exactly the jobs rttnw_render(spp = B, sample_begin = sample_begin + kB) runs for that pixel.
 *   The pixel's running sum is the chain of the passes' chunk-sum chains, in pass order, in the kernels' arithmetic type; its value is
 *   that sum / n_q.  So a pixel that stops after pass 0 is BIT-IDENTICAL to rttnw_render(spp = B), linear value and RGBA8 alike.
 * Noise estimate.  Over the chunk means m_c (n_c samples each) of all chunks of all passes so far, M2 = sum_c n_c (m_c - mu)^2 is folded
 *   with the weighted incremental (West) update in chunk order, in double for every precision, no product fused into an add (every build folds to the same bits); the standard error of
 *   the pixel's mean is sqrt(M2 / ((K - 1) N)), K chunks, N = n_q samples — +inf with K < 2.  Unbiased, the samples being i.i.d. per
 *   pixel; with spp_chunk = 1 it is the textbook sample standard error.
 * Stopping.  After each pass a pixel stays active unless n_q == p->spp or, for each of r, g, b,
 *       stderr <= abs_error + rel_error * value            (linear radiance, value = the pixel's reported mean)
 *   The decision depends on the pixel's own samples only — not on its neighbours, its tile, the launch split (RTTNW_CHUNK_SUM_BUDGET) or
 *   the order jobs are handed out in.  Refinement passes trace the 2x2 pixel blocks that hold an active pixel (a converged pixel of
 *   such a block traces nothing).
 * Padding.  A job group spans 16 chunks of a 2x2 block: with the default schedule (spp_chunk = 0) a pass of B = 32 has 11 chunks,
 *   padded to 16; B = 64 with spp_chunk = 4 is exactly 16 (the Python driver takes spp_chunk = max(1, B / 16) when
 *   given 0).
 * Outputs (each optional; row-major, top row first like rttnw_render): out_linear_rgb w*h*3, out_rgba8 w*h*4, out_spp w*h sample counts
 *   n_q, out_stderr_rgb w*h*3 standard errors of the pixel's mean.  `stats`: samples = sum_q n_q, kernel_ms = device time of all passes
 *   (the per-pass list building and one small copy to the host included), reserved = the kernel form, as for rttnw_render.  Blocking.
 * Refusals, before the device is touched: RTTNW_ERR_INVALID for pass_spp == 0, p->spp not a positive multiple of pass_spp, a negative
 *   or NaN tolerance, reserved0 != 0 or tile_world != 1; RTTNW_ERR_UNSUPPORTED for collect_counters != 0. */
struct rttnw_adaptive {
    uint32_t pass_spp;  /* B: samples per pixel per pass; p->spp (the cap) must be a positive multiple of B */
    uint32_t reserved0; /* must be 0 */
    double rel_error;   /* a pixel stops after the first pass at which, for each of r, g, b, */
    double abs_error;   /*   stderr <= abs_error + rel_error * mean   (linear radiance) */
};
typedef struct rttnw_adaptive rttnw_adaptive;
int rttnw_render_adaptive(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                          double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb,
                          rttnw_stats* stats);

/* First-hit feature buffers ("AOVs") of the frame rttnw_render renders: albedo, normal, depth, coverage — the inputs of a denoiser
 * (rttnw_denoise below, or an external one), an alpha channel, a way to look at a scene.  The reference has no counterpart: its color()
 * (main.rs:26-45) keeps nothing of a path but its radiance.  (Came without a version bump, like rttnw_render_adaptive: detect it by its symbol.)
 *
 * Samples.  For every pixel, samples [sample_begin, sample_begin + spp) start with THE CAMERA RAYS OF rttnw_render (the same keys: pixel,
 *   sample, seed — main.rs:212-215) and do bounce 0 only: world.hit() (main.rs:33) with the keyed draws of bounce 0, so a ConstantMedium in
 *   front (hittable.rs:745-797) decides exactly as it does in the render, and Material::scatter / emitted (main.rs:34-41) at that hit.
 * Per sample.  On a hit: alpha = 1, normal = rec.normal as the hit record holds it (hittable.rs:30-44: against the ray), depth =
 *   rec.t * |ray.direction| (the product formed after the square root, not fused into it or into the sum), albedo = the attenuation if
 *   the material scattered, else what it emitted.  On a miss: alpha = 0, normal = 0, depth = 0, albedo = p->background.
 * Per pixel.  Each channel is ONE chain of additions in sample order in the kernel's arithmetic type, then one division by spp: the
 *   result does not depend on the launch shape.  alpha is fractional and normals are shorter than 1 where a pixel's samples disagree
 *   (silhouettes).  Features over disjoint sample ranges combine like renders do (weights = their spp).
 * p->precision selects the arithmetic build as for rttnw_render (RTTNW_F64_STRICT: the reference's operations, every value within 1e-12 of
 *   the CPU restatement); max_depth and spp_chunk are not used (max_depth must still be valid).  The first call whose camera shutter
 *   reaches outside the trees' interval rebuilds them, and the strict build walks its own lowering, exactly as for rttnw_render.
 * Outputs (each optional; row-major, top row first like rttnw_render; doubles): out_albedo w*h*3, out_normal w*h*3, out_depth w*h,
 *   out_alpha w*h.  `stats`: samples, rays (= samples), kernel_ms, the scene's sizes.  Blocking.
 * Refusals, before the device is touched, in this order: RTTNW_ERR_INVALID for a NULL p, spp == 0, reserved0 != 0 or tile_world != 1;
 *   RTTNW_ERR_UNSUPPORTED for collect_counters != 0; then whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes). */
int rttnw_render_features(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p,
                          double* out_albedo, double* out_normal, double* out_depth, double* out_alpha, rttnw_stats* stats);

/* A window, or a pixel mask, of the frame rttnw_render renders — a preview of the area being worked on, a re-render of a few pixels, one
 * frame split into windows across hosts — at the cost of the selected pixels, not of the frame.  The reference has no counterpart: its
 * render() (main.rs:202-229) always walks the whole image.  (Came without a version bump, like rttnw_render_adaptive: detect it by its symbol.)
 *
 * Frame and window.  The frame is the p->width x p->height frame of rttnw_render, with the same camera and the same keys (pixel, sample,
 *   seed).  The window is its pixels [x0, x1) x [y0, y1), row 0 = top.  `mask` (optional): (x1-x0)*(y1-y0) bytes, row-major, top row first,
 *   nonzero = selected; NULL selects every pixel of the window.
 * Selected pixels.  Samples [sample_begin, sample_begin + spp) under the chunk schedule of spp and spp_chunk, ONE chain of chunk sums in chunk
 *   order, divided by spp: exactly the jobs rttnw_render runs for that pixel.  Its linear value and its RGBA8 are BIT-IDENTICAL to
 *   rttnw_render(s, cam, p) at that pixel — for every `precision`, every kernel form and every launch split (RTTNW_CHUNK_SUM_BUDGET).
 *   The trace runs over the list of 2x2 pixel blocks that hold a selected pixel (an unselected pixel of such a block traces nothing).
 * Unselected pixels of the window.  Linear 0, 0, 0 and RGBA8 0, 0, 0, 0: a rendered pixel has alpha 255, so alpha tells the two apart.
 * Outputs (each optional, sized by the WINDOW; row-major, top row first): out_linear_rgb (x1-x0)*(y1-y0)*3 doubles, out_rgba8
 *   (x1-x0)*(y1-y0)*4 bytes.  Blocking.  `stats`: samples = selected pixels x spp, kernel_ms = device time of everything the call runs (the
 *   list building and one small copy to the host included), reserved = the kernel form, as for rttnw_render; the scene's sizes as usual.
 * All-zero mask.  RTTNW_OK with the outputs cleared and stats->samples == 0; no trace kernel is launched.
 * Memory.  Beyond one selection byte per frame pixel (and the block list: a word per 2x2 block), everything the call allocates is sized by the
 *   listed blocks or by the window: chunk sums 4 per listed block and chunk, running sums 4 per listed block.
 * Refusals, before the device is touched, in this order: RTTNW_ERR_INVALID for a NULL p; RTTNW_ERR_INVALID for x0 >= x1, y0 >= y1,
 *   x1 > width or y1 > height; RTTNW_ERR_INVALID for reserved0 != 0 or tile_world != 1; RTTNW_ERR_UNSUPPORTED for collect_counters != 0 (the
 *   active-list kernels do not tally); then whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes).
 * The first call whose camera shutter reaches outside the trees' interval rebuilds them, and the strict build walks its own lowering,
 *   exactly as for rttnw_render; one render in flight per scene, as before. */
int rttnw_render_region(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p,
                        uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const uint8_t* mask,
                        double* out_linear_rgb, uint8_t* out_rgba8, rttnw_stats* stats);

/* A denoiser for the images above: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the feature buffers of
 * rttnw_render_features and, optionally, by the variance of the pixel means (the colour stop of SVGF, Schied et al. 2017) — the square of
 * rttnw_render_adaptive's out_stderr_rgb.  Host arrays in, host arrays out (row-major, top row first), blocking, on the current device;
 * no scene handle.  No CPU fallback: RTTNW_ERR_HIP without a device.  Everything is double.
 *
 * Demodulation.  A pixel with alpha != 0 is filtered as c = colour / albedo in every channel whose albedo > 1e-3 (c = colour in the others)
 *   and multiplied back at the end; its variance is divided and multiplied by albedo^2 likewise.
 * Passes.  `iterations` passes (0 .. 8), pass i with the 5x5 B3-spline taps h = (1, 4, 6, 4, 1) / 16 at stride 2^i, taps outside the image
 *   dropped, accumulated row-major over the 5x5.  0 iterations copy the input to the output, without demodulation: the identity, bit for bit.
 *   tap weight  w = h_x h_y * w_n * w_z * w_l; taps whose alpha is 0 are dropped, and a centre whose alpha is 0 passes through unchanged
 *     w_n = max(0, n . n')^E              E = the smallest power of two >= sigma_normal (at most 1024), by repeated squaring
 *     w_z = r^2,  r = 1 / (1 + (dz / (sigma_depth * (|z| + |z'|) / 2 + 1e-12))^2)
 *     w_l = 1 / (1 + (dlum / (sigma_luminance * sqrt(max(V, 0)) + 1e-12))^2)    lum = 0.2126 r + 0.7152 g + 0.0722 b of c;  w_l = 1 when
 *           variance_rgb == NULL or the centre's variance is not finite (in any channel).  V = the variance of the centre's luminance
 *           (0.2126^2 var_r + ...) averaged over its 3x3 neighbourhood with taps (1, 2, 1) x (1, 2, 1), dropping taps outside the image,
 *           with alpha == 0 or with a variance that is not finite
 *     alpha, normal and albedo are sample means: alpha is fractional and normals are shorter than 1 on silhouettes; the weights take
 *     them as they are.
 *   colour = sum w c / sum w;  variance = sum w^2 var / (sum w)^2 over the taps whose variance is finite (a centre whose own variance is
 *   not finite keeps it), both carried to the next pass.  A centre all of whose taps weigh 0 passes through.
 * No transcendental function anywhere: + - * /, sqrt and comparisons only, no product fused into a sum, so the device code, a host build
 *   of the same header (rttnw_amd/csrc/denoise.hpp) and a restatement in numpy give the same bits.
 * Parameters.  A sigma of 0 means the library default: sigma_luminance 4 (SVGF's), sigma_normal 64 (|n . n'| = 0.99, 8 degrees, weighs
 *   0.53), sigma_depth 0.1 (a tap 10 % nearer or farther weighs 0.25, 30 %: 0.01).  DESIGN.md section 10b says how they were chosen.
 * Outputs: out_linear_rgb w*h*3 (optional), out_rgba8 w*h*4 after main.rs:219-225 (optional), out_variance_rgb w*h*3 (optional; written
 *   only when variance_rgb was given), kernel_ms (optional): device time of the passes.
 * Refusals, before the device is touched: RTTNW_ERR_INVALID for a NULL linear_rgb, albedo, normal, depth, alpha or d, width * height == 0,
 *   iterations > 8, reserved0 != 0, a negative or NaN sigma. */
struct rttnw_denoise_params {
    uint32_t iterations; /* 0 .. 8; 5 reaches 2 * 16 = 32 pixels to either side */
    uint32_t reserved0;  /* must be 0 */
    double sigma_luminance, sigma_normal, sigma_depth; /* 0 = the library default */
};
typedef struct rttnw_denoise_params rttnw_denoise_params; /* (not `rttnw_denoise`: in C a typedef and a function share one name space) */
int rttnw_denoise(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb,
                  const double* albedo, const double* normal, const double* depth, const double* alpha,
                  const rttnw_denoise_params* d, double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb,
                  double* kernel_ms);

/* A second denoiser, which reads NO feature buffer: non-local means over two half-buffers (Rousselle, Knaus and Zwicker 2012, "Adaptive
 * rendering with non-local means filtering").  rttnw_denoise is steered by the first hit; what a mirror shows, what lies behind glass, a
 * procedural texture on one surface is not in first-hit features.  Here the weights come from the colour itself:
 * half_a and half_b are the means of two disjoint, equally large sample sets of one frame (two rttnw_render calls of spp / 2 samples at
 * sample_begin and sample_begin + spp / 2), small patches of pixels are compared in ONE half, and the weights found there average the OTHER
 * half — so no weight depends on the noise it averages.  Calling convention as rttnw_denoise: host arrays in and out (row-major, top row
 * first), blocking, on the current device, no scene handle; no CPU fallback: RTTNW_ERR_HIP without a device.  Everything is double.
 *
 * Coordinates.  A value "at" a coordinate outside the image is the value of the nearest pixel inside: every coordinate below — patch taps,
 *   candidates, the taps of the variance's 3x3 — is clamped to the image on its own (x = clamp(p + n), q = clamp(p + n + o)).
 * Variance.  V_a, V_b are the guides' variances: var_a and var_b (the variance of each half's pixel MEAN) when given; otherwise both are the
 *   pair variance, per channel  V(x) = (sum over the 3x3 around x, row-major, of (a - b)^2 * 0.5) / 9.
 * Pixel distance in guide g with variance V, for offset o, q = x + o, per channel c:
 *     delta_c(x, o) = ((g_x - g_q)^2 - (V_x + min(V_x, V_q))) / (1e-10 + k^2 * (V_x + V_q))          k^2 = k * k, rounded once
 *     delta(x, o)   = (delta_r + delta_g) + delta_b                    the sum over the channels; their mean is taken with the patch's
 * Patch distance.  R(x, o) = sum over nx = -f .. f, left to right, of delta(x + (nx, 0), o): the row sums;
 *     D(p, o) = (sum over ny = -f .. f, top to bottom, of R(p + (0, ny), o)) / (3 * (2f + 1)^2): the mean over channels and patch taps.
 * Weight.  t = 1 / (1 + 0.25 * m), m = 0 where D < 0 and D otherwise;  w = (t * t) * (t * t).  The centre offset weighs exactly 1, whatever
 *   its D, so the sum of weights is never 0.
 * Cross filtering.  a'(p) = (sum_o w_B(p, o) * a(p + o)) / (sum_o w_B(p, o)) with the weights of guide b and V_b, over the (2r+1)^2 offsets
 *   row-major (oy outer, ox inner); b'(p) likewise with the weights of guide a and V_a.
 * Outputs (each optional): out_linear_rgb w*h*3 = (a' + b') * 0.5; out_rgba8 w*h*4 of it after main.rs:219-225, alpha 255; out_half_a and
 *   out_half_b w*h*3 = a' and b'; out_error_rgb w*h*3 = (a' - b')^2 * 0.25, an estimate of the output's variance; kernel_ms: device time of
 *   the call's kernels.
 * Every sum starts from 0.0 and adds its terms in the order stated; no product is fused into a sum; + - * / and comparisons only, no
 *   transcendental function (the square root of the RGBA8 output aside).  So the device code, a host build of the same header
 *   (rttnw_amd/csrc/nlm.hpp) and a restatement in numpy give the same bits.  Swapping (half_a, var_a) with (half_b, var_b) swaps out_half_a
 *   with out_half_b and leaves the other outputs bit-identical.  A pixel's outputs depend on the inputs within r + f + 1 pixels of it only.
 * Non-finite values.  A value or a variance that is not finite is not special-cased: it propagates through every sum it enters (D < 0 is
 *   false for a NaN, so a NaN distance makes a NaN weight).
 * Parameters.  0 means the library default: search_radius 7 (15x15 candidates), patch_radius 3 (7x7 patches), k 0.7.
 * Refusals, before the device is touched, each message naming denoise_nlm and the argument: RTTNW_ERR_INVALID for a NULL half_a, half_b or
 *   d, exactly one of var_a / var_b, width * height == 0, search_radius > 16, patch_radius > 4, a reserved field that is not 0, a negative
 *   or NaN k.
 * Out of scope: multiplying the first-hit normal and depth stops into the weight, albedo demodulation, steering the adaptive rounds by
 *   out_error_rgb, a node-wide form. */
struct rttnw_nlm_params {
    uint32_t search_radius; /* r: candidates q = p + o, o in [-r, r]^2; 0 = default 7; 1 .. 16 */
    uint32_t patch_radius;  /* f: (2f+1)^2 patch; 0 = default 3; 1 .. 4 */
    double k;               /* distance scale; 0 = default 0.7; negative or NaN refused */
    uint32_t reserved0, reserved1; /* must be 0 */
};
typedef struct rttnw_nlm_params rttnw_nlm_params;
int rttnw_denoise_nlm(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a,
                      const double* var_b, const rttnw_nlm_params* d, double* out_linear_rgb, uint8_t* out_rgba8,
                      double* out_half_a, double* out_half_b, double* out_error_rgb, double* kernel_ms);

/* A choice, per pixel, between the two denoisers above.  rttnw_denoise wins where the first hit describes the surface (a wall's normal and
 * depth say "same surface" with no noise at all), rttnw_denoise_nlm where it does not (a procedural texture, what a mirror shows); a real frame
 * holds both kinds of region (DESIGN.md section 10b has the measurements).  The two halves are independent estimates of one frame, so a
 * filtered half can be scored against the OTHER, raw half: that half's own noise enters both filters' scores alike and cancels in their
 * difference.  This is the selection step of Rousselle, Knaus and Zwicker 2012.  Calling convention as the two filters: host arrays in and out
 * (row-major, top row first), blocking, on the current device, no scene handle; no CPU fallback: RTTNW_ERR_HIP without a device.  Everything is
 * double.  a, b are half_a, half_b.
 *
 * 1. Feature-guided halves.  Fa = the out_linear_rgb of rttnw_denoise(half_a, var_a or NULL, albedo, normal, depth, alpha, dn), Fb = the same of
 *    half_b and var_b: bit for bit what that entry point returns.
 * 2. Non-local-means halves.  Na, Nb = out_half_a, out_half_b of rttnw_denoise_nlm(half_a, half_b, var_a, var_b, nl), bit for bit.
 * 3. Cross-validated error, per pixel.  For channel c  tF_c = (Fa_c - b_c) * (Fa_c - b_c) + (Fb_c - a_c) * (Fb_c - a_c);
 *    E_F = (tF_r + tF_g) + tF_b;  E_N likewise from Na, Nb;  d = (E_F - E_N) / (1e-10 + (E_F + E_N)), a value in [-1, 1]: normalised, so that
 *    a bright region's errors do not outvote its neighbours inside the window.
 * 4. Window sum.  Coordinates are clamped to the image, each on its own, as in rttnw_denoise_nlm.  R(x, y) = sum over ox = -s .. s, left to
 *    right, of d(clamp(x + ox), y);  S(p) = sum over oy = -s .. s, top to bottom, of R(x, clamp(y + oy)); both sums start from 0.0.
 *    m(p) = 1.0 where S(p) > margin * double((2s+1)^2) (the product rounded once), otherwise 0.0: a NaN S compares false and chooses the
 *    feature-guided filter.
 * 5. Blend weight.  beta(p) = (the same two-stage clamped sum of m with radius t) / double((2t+1)^2): a window of all ones gives exactly
 *    1.0, a window of all zeros exactly 0.0.
 * 6. Output.  F_c = (Fa_c + Fb_c) * 0.5, N_c = (Na_c + Nb_c) * 0.5.  blend(n, f) = f where beta == 0, n where beta == 1, otherwise
 *    beta * n + (1.0 - beta) * f: two products and one sum, not fused.  The branches keep a non-finite value of the filter that was not
 *    chosen out of the pixel (with t <= s, a NaN d makes m 0 on every pixel of its blend window, so beta is exactly 0 there; a blend window
 *    wider than the error window can reach past that).  out_linear_rgb w*h*3 = blend(N_c, F_c); out_rgba8 w*h*4 of it after main.rs:219-225, alpha 255; out_blend
 *    w*h = beta; out_feature_rgb w*h*3 = F; out_nlm_rgb w*h*3 = N; out_error_rgb w*h*3 = (A_c - B_c) * (A_c - B_c) * 0.25 with
 *    A_c = blend(Na_c, Fa_c), B_c = blend(Nb_c, Fb_c): the analogue of rttnw_denoise_nlm's error output; kernel_ms: device time of every
 *    kernel of the call.  Each output is optional.
 * 7. Arithmetic.  + - * / and comparisons only in steps 3 to 6 (the square root of the RGBA8 output aside); no product is fused into a sum;
 *    every sum adds its terms in the order stated.  So the device code, a host build of the same header (rttnw_amd/csrc/select.hpp) and a
 *    restatement in numpy give the same bits.  Swapping (half_a, var_a) with (half_b, var_b) leaves every output bit-identical.  A pixel's
 *    outputs depend on the inputs within max(r + f + 1, 2 * (2^iterations - 1)) + s + t pixels of it only.
 * Parameters.  error_radius 0 = 5, blend_radius 0 = 2.  A margin of 0 is meaningful (the filter with the smaller summed error wins), so the
 *   default margin has a flag of its own: use_default_margin != 0 takes 0.01 and ignores `margin`.  DESIGN.md section 10b says why it is not 0.
 *   margin 2 chooses the feature-guided filter everywhere (S <= (2s+1)^2 always), margin -2 non-local means everywhere a window holds no NaN.
 * Refusals, before the device is touched, each message naming denoise_select and the argument: RTTNW_ERR_INVALID for everything the two
 *   filters refuse for their own arguments — a NULL half_a, half_b, albedo, normal, depth, alpha, dn or nl, exactly one of var_a / var_b,
 *   width * height == 0, dn->iterations > 8, dn->reserved0 != 0, a negative or NaN sigma, nl->search_radius > 16, nl->patch_radius > 4, a
 *   reserved field of nl that is not 0, a negative or NaN nl->k — and for a NULL sel, error_radius > 16, blend_radius > 8, a margin outside
 *   [-2, 2] or NaN (where it is not ignored), sel->reserved0 != 0.
 * Out of scope: steering the adaptive rounds by out_blend or out_error_rgb, a node-wide form, the native rttnw program, a third candidate
 *   filter. */
struct rttnw_select_params {
    uint32_t error_radius;  /* s: the error difference is summed over (2s+1)^2 pixels; 0 = default 5; 1 .. 16 */
    uint32_t blend_radius;  /* t: the binary choice is averaged over (2t+1)^2 pixels; 0 = default 2; 1 .. 8 */
    double margin;          /* tau in [-2, 2]: non-local means is chosen where the mean normalised error difference exceeds it */
    uint32_t use_default_margin, reserved0; /* use_default_margin != 0: margin is ignored and 0.01 is used; reserved0 must be 0 */
};
typedef struct rttnw_select_params rttnw_select_params;
int rttnw_denoise_select(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a,
                         const double* var_b, const double* albedo, const double* normal, const double* depth, const double* alpha,
                         const rttnw_denoise_params* dn, const rttnw_nlm_params* nl, const rttnw_select_params* sel,
                         double* out_linear_rgb, uint8_t* out_rgba8, double* out_blend, double* out_feature_rgb, double* out_nlm_rgb,
                         double* out_error_rgb, double* kernel_ms);

/* A third spatial filter, which joins the two above: weighted first-order regression of colour on the first-hit features (Moon, Carr and Yoon
 * 2014, "Adaptive rendering based on weighted local regression"; Bitterli et al. 2016, "Nonlinearly weighted first-order regression for
 * denoising Monte Carlo renderings").  The weights are rttnw_denoise_nlm's, cross-filtered, so no weight depends on the noise it averages; but
 * where non-local means fits a CONSTANT to the candidates of a pixel, this fits a local linear model of colour in the features (albedo,
 * normal, depth of rttnw_render_features) and keeps only the intercept.  A constant fit blurs whatever the features explain — a texture, a
 * shading gradient across a curved surface, a depth ramp; the first-order fit does not.  With demodulation the colour is divided by the albedo
 * before the weights are measured, as rttnw_denoise does.  The calling convention is rttnw_denoise_nlm's: host arrays in and out (row-major,
 * top row first), blocking, on the current device, no scene handle; no CPU fallback: RTTNW_ERR_HIP without a device.  Everything is double;
 * every output is optional.  half_a, half_b, var_a, var_b as for rttnw_denoise_nlm; albedo, normal w*h*3, depth, alpha w*h.
 *
 * Arithmetic rules.  Every product is rounded on its own (none is fused into a sum), every sum starts from 0.0 and adds its terms in the order
 *   stated, and only + - * /, sqrt and comparisons are used.  So the device code, a host build of the same header
 *   (rttnw_amd/csrc/regress.hpp) and a restatement in numpy give the same bits.
 * 1. Demodulation (demodulate != 0; needs albedo and alpha).  For a pixel with alpha != 0 and a channel with albedo > 1e-3 (rttnw_denoise's
 *    rule and constant) a and b are divided by the albedo, and given variances by albedo * albedo (the product rounded once).  The pair variance,
 *    when no variances are given, is formed from the demodulated halves.  Steps 2 to 5 run on these arrays.  At the end a' and b' are
 *    multiplied by the centre's albedo in the same channels, before step 6.
 * 2. Weights.  w_B(p, o) and w_A(p, o) are exactly rttnw_denoise_nlm's, with its coordinates, clamping and pair variance unchanged; the offsets
 *    run row-major (oy outer, ox inner) and the centre weight is 1.
 * 3. Regressors.  The pixel's feature mask m is `features`, or 0 when the centre's alpha == 0.  With m == 0 no feature array is read for that
 *    pixel and no candidate is dropped.  With m != 0 a candidate whose clamped pixel has alpha == 0 is dropped: it enters no sum.  x(q) holds
 *    the selected components in the order albedo r g b, normal x y z, depth; each is feature(q) - feature(p) as stored, except the depth
 *    component, which is (z_q - z_p) / z_p with z = depth / alpha.  d is the number of components: 0, 1, 3, 4, 6 or 7.
 * 4. Sums, over the kept candidates in offset order, y the other half's colour at the candidate (the half being fitted), c = 0 .. 2:
 *      s = s + w;  t_c = t_c + w * y_c                      (rttnw_denoise_nlm's two sums)
 *      wx_i = w * x_i, formed once per candidate and component;  b_i = b_i + wx_i;  A_ij = A_ij + wx_i * x_j for j <= i;  C_ic = C_ic + wx_i * y_c
 *    After the loop: A_ii = A_ii + ridge * s.
 * 5. Solve: the features first, the constant eliminated last.  Cholesky row by row: for j = 0 .. d-1 and i = 0 .. j: acc = A_ji, then
 *    acc = acc - L_jk * L_ik for k = 0 .. i-1 in order; when i < j: L_ji = acc / L_ii; when i == j: the pivot test acc > 0 must hold, and
 *    L_jj = sqrt(acc).  Forward substitution, k in order: u_j = (b_j - sum_k L_jk u_k) / L_jj, and G_jc likewise from C_jc.
 *    uu = sum_j u_j * u_j, uG_c = sum_j u_j * G_jc, den = s - uu.  The fitted value at p is (t_c - uG_c) / den.
 *    Fallback.  The pixel falls back when a pivot test is false (this includes a NaN) or when den >= 0.5 is false.  In exact arithmetic
 *    den >= 1 (the centre has weight 1 and x = 0; the rest is Cauchy-Schwarz), so a smaller den means the solve lost its accuracy.  The
 *    fallback is the zero-order value t_c / s, over the same kept candidates.  With d == 0 the formulas reduce to t_c / s exactly:
 *    uu = uG = 0.0.
 * 6. Outputs.  a' uses w_B and regresses half a; b' uses w_A and regresses half b.  out_half_a and out_half_b w*h*3 hold a' and b';
 *    out_linear_rgb w*h*3 = (a' + b') * 0.5, out_rgba8 w*h*4 of it after main.rs:219-225, alpha 255, and out_error_rgb w*h*3 =
 *    (a' - b')^2 * 0.25, as rttnw_denoise_nlm forms them; out_fit w*h holds 0.0, 1.0 or 2.0: how many of the two directions used the
 *    first-order value; kernel_ms: device time of the call's kernels.
 * 7. Properties.  (1) With features == 0 and demodulate == 0 every output of rttnw_denoise_nlm is reproduced bit for bit, and the four feature
 *    arrays may be NULL.  (2) Swapping (half_a, var_a) with (half_b, var_b) swaps out_half_a with out_half_b and leaves the other outputs
 *    bit-identical.  (3) A pixel's outputs depend on the inputs within r + f + 1 pixels of it only.  (4) Non-finite inputs are not
 *    special-cased beyond the two tests of step 5.
 * Parameters.  search_radius, patch_radius and k as rttnw_nlm_params (0 = 7, 3, 0.7).  ridge 0 = the library default, 1e-1 (DESIGN.md
 *   section 10b has the sweep it was taken from).  features has no default: 0 is meaningful.
 * Refusals, before the device is touched, in this order, each message naming denoise_regress and the argument: RTTNW_ERR_INVALID for
 *   everything rttnw_denoise_nlm refuses — a NULL half_a or half_b — and a NULL g; exactly one of var_a / var_b; width * height == 0;
 *   search_radius > 16; patch_radius > 4; a negative or NaN k; features > 7; a negative or NaN ridge; a non-zero reserved field;
 *   features != 0 with a NULL array among those it selects — alpha whenever features != 0, albedo with bit 1, normal with bit 2, depth with
 *   bit 4; demodulate != 0 with a NULL albedo or alpha.
 * Out of scope: offering this filter to rttnw_denoise_select as a third candidate, prefiltering the features, a second-order or
 *   per-channel-bandwidth fit, steering the adaptive rounds by out_error_rgb or out_fit, the SVGF handle (which now lives below, at
 *   rttnw_svgf_set_regress), a node-wide form, the native rttnw
 *   program. */
struct rttnw_regress_params {
    uint32_t search_radius, patch_radius; /* r, f: as rttnw_nlm_params; 0 = 7, 3; r <= 16, f <= 4 */
    double k;                             /* as rttnw_nlm_params; 0 = 0.7 */
    double ridge;                         /* lambda; 0 = the library default; negative or NaN refused */
    uint32_t features;                    /* bits: 1 albedo (3 regressors), 2 normal (3), 4 depth (1); 0 .. 7, no default: 0 is meaningful */
    uint32_t demodulate;                  /* != 0: filter colour / albedo */
    uint32_t reserved0, reserved1;        /* must be 0 */
};                                        /* 40 bytes, offsets 0 4 8 16 24 28 32 36 */
typedef struct rttnw_regress_params rttnw_regress_params;
int rttnw_denoise_regress(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                          const double* albedo, const double* normal, const double* depth, const double* alpha, const rttnw_regress_params* g,
                          double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb,
                          double* out_fit, double* kernel_ms);

/* Temporal accumulation: this frame blended with the previous call's result, fetched from where each pixel's surface point was in the previous
 * frame.  The scene is static and the camera moves (a turntable, a fly-through), so the point behind a pixel was, almost always, seen by the
 * previous frame as well: its accumulated colour is more samples per pixel at no trace cost.  This is the temporal stage of SVGF (Schied et al.
 * 2017), whose spatial half is rttnw_denoise.  Calling convention as rttnw_denoise: host arrays in and out (row-major, top row first), blocking,
 * on the current device, no scene handle; no CPU fallback: RTTNW_ERR_HIP without a device.  Everything is double.
 *
 * Arrays.  linear_rgb w*h*3, normal w*h*3, depth w*h, alpha w*h: this frame's render and its rttnw_render_features maps (depth is the distance
 *   from the ray origin to the first hit, summed over the samples that hit and divided by all samples, like alpha).  prev_linear_rgb,
 *   prev_variance_rgb, prev_length: the previous call's out_linear_rgb, out_variance_rgb, out_length; prev_normal, prev_depth, prev_alpha: the
 *   previous frame's feature maps.  prev_length w*h: the frames a pixel's history counts; 0 means "no history here".
 * Cameras.  Both descriptors become the camera record the renders use (Camera::new, camera.rs:32-61): origin o, lower_left_corner llc,
 *   horizontal H, vertical V; subscript p marks the previous frame's.  The arithmetic below starts from those records.  The lens is taken at its
 *   centre: an aperture above 0 is ignored.  Shutter times are not read.
 * No history.  prev_linear_rgb, prev_variance_rgb, prev_length, prev_normal, prev_depth and prev_alpha all NULL (prev_cam may then be NULL):
 *   every pixel gets out = this frame, out_length 1, the variance copied, out_prev_xy NaN.
 * A pixel with alpha == 0 passes through the same way (colour and variance copied, length 1, out_prev_xy NaN): the background is exact there.
 * 1. Where the pixel was.  dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2, everywhere.  For pixel (x, y) with alpha != 0, component by component:
 *    s = (x + 0.5) / w;  t = ((h - 1 - y) + 0.5) / h;  d = ((llc + s * H) + t * V) - o;  z = depth / alpha, the mean distance of the samples
 *    that hit;  P = o + d * (z / sqrt(dot(d, d))).  Against the previous record:  q = P - o_p;  n = H_p x V_p, that is
 *    (H1 * V2 - H2 * V1, H2 * V0 - H0 * V2, H0 * V1 - H1 * V0);  e = llc_p - o_p;  lambda = dot(e, n) / dot(q, n);  r = lambda * q - e;
 *    s' = dot(r, H_p) / dot(H_p, H_p);  t' = dot(r, V_p) / dot(V_p, V_p);  fx = s' * w - 0.5;  fy = (h - t' * h) - 0.5;  zq = sqrt(dot(q, q)).
 *    The pixel has no history (out = this frame, length 1, out_prev_xy NaN) when lambda > 0 is false, when fx or fy is not finite, or when
 *    -1 < fx < w or -1 < fy < h is false.  Otherwise out_prev_xy = (fx, fy) — also when every tap below is rejected: the output doubles as a
 *    motion-vector map.
 * 2. Bitwise-equal cameras.  When the 15 doubles of the two descriptors are bitwise equal the geometry is skipped: fx = x, fy = y, zq = z
 *    exactly, so a static camera accumulates pixel on pixel, with no bilinear blur (the general formulas leave a residual of 1e-14 pixels).
 * 3. Taps.  x0 = floor(fx), ax = fx - x0, y0 = floor(fy), ay = fy - y0.  The four taps (x0 + i, y0 + j) have weights
 *    (i ? ax : 1 - ax) * (j ? ay : 1 - ay) and are visited in the order 00, 10, 01, 11 (i first).  A tap is dropped when it lies outside the
 *    image, when its prev_alpha == 0, when its prev_length > 0 is false, when abs(prev_depth / prev_alpha - zq) <= depth_tolerance * zq is
 *    false, or when dot(n, n') >= normal_min * sqrt(dot(n, n) * dot(n', n')) is false — n this pixel's normal, n' the tap's, both as stored:
 *    stored normals are short on silhouettes, hence the normalised test.  With normal_min == -1 the normal test is not made.
 * 4. Blend.  Every sum starts from 0.0 and adds the accepted taps in the order of step 3.  W = the sum of the accepted weights.  W > 0 false:
 *    reset — out = this frame, length 1, the variance copied.  Otherwise hist = (sum w * c') / W per channel, L = (sum w * len') / W and, with
 *    variances, vh = (sum w * var') / W: the plain weighted mean, because an accumulated history's taps are correlated and the independent-tap
 *    formula would understate it.  N = min(L + 1, double(max_history)) (L + 1 where it is the smaller, otherwise — a NaN too — max_history);
 *    a = 1.0 / N;  out = (1 - a) * hist + a * cur: two products and one sum, not fused;  out_var = ((1 - a) * (1 - a)) * vh + (a * a) * var;
 *    out_length = N.  Non-finite colours and variances are not special-cased: they propagate through the sums they enter.
 * 5. Outputs, each optional: out_linear_rgb w*h*3; out_rgba8 w*h*4 of it after main.rs:219-225, alpha 255; out_variance_rgb w*h*3, written
 *    only when variance_rgb was given; out_length w*h; out_prev_xy w*h*2 (fx, fy); kernel_ms: device time of the kernel alone.
 * 6. Arithmetic.  + - * /, sqrt, floor, abs and comparisons only; no product is fused into a sum; every expression is evaluated in the order
 *    written above.  So the device code, a host build of the same header (rttnw_amd/csrc/temporal.hpp) and a restatement in numpy give the
 *    same bits.
 * Variances.  variance_rgb (of this frame's pixel means) is optional; beside a history variance_rgb and prev_variance_rgb come both or neither.
 * Refusals, before the device is touched, each message naming temporal_accumulate and the argument: RTTNW_ERR_INVALID for a NULL cam,
 *   linear_rgb, normal, depth, alpha or t, width * height == 0, some but not all of the prev_* arrays, a history with a NULL prev_cam, exactly
 *   one of variance_rgb / prev_variance_rgb beside a history, max_history > 65535, reserved0 != 0, a negative or NaN depth_tolerance, a
 *   normal_min that is NaN or outside [-1, 1].
 * Out of scope: moving geometry beyond what one shutter interval blurs; reflections and refractions, which are reprojected with their surface
 *   and will ghost (SVGF's known limit); albedo demodulation of the history; feeding the filtered image back into the history; colour
 *   clamping; a device-resident chain between frames; a node-wide form; the native rttnw program. */
struct rttnw_temporal_params {
    uint32_t max_history;    /* the most frames a pixel's history counts; 0 = default 32; 1 .. 65535 */
    uint32_t reserved0;      /* must be 0 */
    double depth_tolerance;  /* relative; 0 = default 0.05; negative or NaN refused */
    double normal_min;       /* in [-1, 1]; 0 = default 0.9; -1 switches the test off; NaN or outside refused */
};
typedef struct rttnw_temporal_params rttnw_temporal_params;
int rttnw_temporal_accumulate(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam,
                              const double* linear_rgb, const double* variance_rgb, const double* normal, const double* depth,
                              const double* alpha, const double* prev_linear_rgb, const double* prev_variance_rgb,
                              const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                              const rttnw_temporal_params* t, double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb,
                              double* out_length, double* out_prev_xy, double* kernel_ms);

/* Temporal accumulation with a variance estimate: rttnw_temporal_accumulate's blend, the second moment of the colour carried along the same
 * reprojected history, and from the two moments the variance of each pixel's accumulated mean — the variance estimation of SVGF (Schied et al.
 * 2017, section 4.2), the piece between its temporal stage and its spatial one.  A sequence of plain renders has no per-pixel variance; this
 * call makes one from the frame history, and where the history is too short to trust (a disoccluded pixel, the first frames) from a window of
 * neighbours guided by normal and depth.  Calling convention as rttnw_temporal_accumulate: host arrays in and out (row-major, top row first),
 * blocking, on the current device, no scene handle; no CPU fallback: RTTNW_ERR_HIP without a device.  Everything is double.
 *
 * Arrays.  linear_rgb, normal, depth, alpha, prev_linear_rgb, prev_length, prev_normal, prev_depth, prev_alpha and the two cameras: as
 *   rttnw_temporal_accumulate.  prev_moment2_rgb w*h*3: the previous call's out_moment2_rgb.  No history: all six prev_* arrays NULL,
 *   prev_moment2_rgb among them (prev_cam may then be NULL).
 * Stage A, accumulate.  Steps 1 - 4 of rttnw_temporal_accumulate are followed without variances: out_linear_rgb, out_rgba8, out_length and
 *   out_prev_xy are bit-identical to that entry point's for the same inputs.  A third quantity rides on the same accepted taps, in the same
 *   order and with the same weights wt: h2 = (sum wt * m2') / W per channel, m2' the tap's prev_moment2_rgb.  With s = cur * cur (rounded once)
 *   out_m2 = (1 - a) * h2 + a * s: two products and one sum, not fused.  out_m2 = s in every case in which the colour passes through: no
 *   history, alpha == 0, no place in the previous frame, W > 0 false.
 * Stage B, estimate.  It reads stage A's outputs — m1 = out_linear_rgb, m2 = out_m2, N = out_length — and this frame's normal, depth and
 *   alpha.  pos(x) = x < 0 ? 0 : x, so a NaN stays a NaN.  Per pixel and channel:
 *   alpha == 0: var = 0 — the background is exact.
 *   N >= min_temporal: var = pos(m2 - m1 * m1) / (N - 1).  m2 - m1 * m1 is the biased per-frame variance of N frame values; times N / (N - 1) it
 *     is unbiased, and over N it is the variance of their mean.
 *   Otherwise the spatial estimate, over the window dy = -radius .. radius (outer), dx = -radius .. radius (inner), the centre among the taps.
 *     Taps outside the image, or whose alpha == 0, are dropped.  A tap weighs w = w_n * w_z, rttnw_denoise's two feature weights in its
 *     expressions, n and z the centre's normal and depth, n' and z' the tap's, both as stored:
 *       w_n = (n0 * n'0 + n1 * n'1) + n2 * n'2, replaced by 0 where w_n > 0 is false, then squared k times, 2^k the smallest power of two
 *         >= sigma_normal (k at most 10);
 *       qz = (z - z') / ((sigma_depth * (abs(z) + abs(z'))) * 0.5 + 1e-12);  r = 1 / (1 + qz * qz);  w_z = r * r.
 *     There is no B-spline factor and no colour stop.  Sw = sum w;  M1 = (sum w * m1') / Sw;  M2 = (sum w * m2') / Sw;
 *     var = pos(M2 - M1 * M1) / N.  Sw > 0 false: var = pos(m2 - m1 * m1) / N.
 * Arithmetic.  Every sum starts from 0.0 and adds in the order stated; no product is fused into a sum; only + - * /, the functions stage A
 *   already uses, and comparisons.  Non-finite values are not special-cased: they propagate through the sums they enter.  So the device code, a
 *   host build of the same header (rttnw_amd/csrc/variance.hpp) and a restatement in numpy give the same bits.
 * out_variance_rgb is the variance of the pixel means in rttnw_denoise's sense and can be handed to it as variance_rgb.
 * Outputs, each optional: out_linear_rgb w*h*3, out_rgba8 w*h*4, out_length w*h, out_prev_xy w*h*2 as rttnw_temporal_accumulate's;
 *   out_moment2_rgb w*h*3; out_variance_rgb w*h*3; kernel_ms: device time of both kernels.
 * Refusals, before the device is touched, each message naming temporal_variance and the argument: RTTNW_ERR_INVALID for everything
 *   rttnw_temporal_accumulate refuses for the arguments they share (a NULL cam, linear_rgb, normal, depth, alpha or t, width * height == 0, a
 *   history with a NULL prev_cam, t's fields), some but not all of the six prev_* arrays, a NULL v, min_temporal == 1 or > 65535, radius > 4, a
 *   reserved field that is not 0, a negative or NaN sigma.
 * Out of scope: albedo-demodulated moments — a texture inside the window reads as variance, SVGF's known overestimate; luminance-only
 *   moments; a device-resident chain between frames; feeding the filtered image back into the history; a node-wide form; the native rttnw
 *   program. */
struct rttnw_variance_params {
    uint32_t min_temporal;  /* a history of at least this many frames is trusted; 0 = default 4; 2 .. 65535 */
    uint32_t radius;        /* the spatial window is (2 radius + 1)^2; 0 = default 3; 1 .. 4 */
    double sigma_normal, sigma_depth; /* as rttnw_denoise_params: 0 = that filter's defaults (64, 0.1) */
    uint32_t reserved0, reserved1;    /* must be 0 */
};
typedef struct rttnw_variance_params rttnw_variance_params;
int rttnw_temporal_variance(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam,
                            const double* linear_rgb, const double* normal, const double* depth, const double* alpha,
                            const double* prev_linear_rgb, const double* prev_moment2_rgb, const double* prev_length,
                            const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                            const rttnw_temporal_params* t, const rttnw_variance_params* v,
                            double* out_linear_rgb, uint8_t* out_rgba8, double* out_moment2_rgb, double* out_length, double* out_prev_xy,
                            double* out_variance_rgb, double* kernel_ms);

/* The SVGF loop on the device: one handle that owns a sequence's history on the device, and one call per frame that runs render, features,
 * accumulate, estimate, filter and feed back on it — rttnw_temporal_variance, rttnw_temporal_accumulate and rttnw_denoise joined without the
 * host between them, with the two things their own scope left out: the filtered image fed back into the colour history, and albedo
 * demodulation of everything the history holds.  rttnw_svgf_push takes a frame the caller rendered, as host arrays (row-major, top row first)
 * like rttnw_temporal_variance; rttnw_svgf_frame renders it itself — rttnw_render's trace (one rank, every precision) and
 * rttnw_render_features' pass at feature_spp samples and the same sample_begin — and neither result leaves the device.  The handle belongs to the
 * device that is current at rttnw_svgf_create; every buffer, ping-pong state included, is allocated there and then, and the estimate kernel's
 * dynamic LDS is admitted: the handle's own stages allocate nothing in a frame call (the trace and the feature pass keep the workspaces they have
 * in rttnw_render and rttnw_render_features), run on one stream, and the call waits once behind them, before it copies out the outputs the caller
 * asked for; an output that is NULL is not copied.  No CPU fallback: rttnw_svgf_create returns RTTNW_ERR_HIP without a device.  Everything
 * behind the trace is double.
 *
 * The contract is a composition of the existing entry points.  The state after a call is {H, M1, M2, L, the frame's normal / depth / alpha, its
 * camera}; it is empty after rttnw_svgf_create and after rttnw_svgf_reset.  In a call the frame has colour C, features F and camera cam; cam' is
 * the state's camera.
 * 0. Demodulate, only with `demodulate`.  For a pixel with alpha != 0 and a channel whose albedo > 1e-3, c = C / albedo — rttnw_denoise's rule;
 *    everywhere else c = C.  A1 is an albedo map of all 1.0.  Without `demodulate` c = C and A1 = F.albedo.
 * 1. Accumulate and estimate.  TV = rttnw_temporal_variance(cam, cam', c, F, prev_linear_rgb = M1, prev_moment2_rgb = M2, prev_length = L, the
 *    state's normal, depth and alpha, t, v); with an empty state the no-history call.  The new M1, M2 and L, prev_xy and var are its
 *    out_linear_rgb, out_moment2_rgb, out_length, out_prev_xy and out_variance_rgb, bit for bit.
 * 2. Colour history.  With feedback_iterations > 0 and a state, A = rttnw_temporal_accumulate(cam, cam', c, no variances, F, prev_linear_rgb = H,
 *    prev_length = L, the state's normal, depth and alpha, t).out_linear_rgb; its length and prev_xy are TV's, bit for bit: the taps are the same
 *    (on the device they are computed once and carry the three quantities).  Otherwise A = M1.
 * 3. Filter.  D, Dv = the out_linear_rgb and out_variance_rgb of rttnw_denoise(A, var, A1, F.normal, F.depth, F.alpha, d).
 * 4. Feed back.  With feedback_iterations = j > 0 the new H is the out_linear_rgb of the same rttnw_denoise call with iterations = j.  A pass
 *    does not depend on how many follow it: on the device this is a tap of the pass loop, not a second run.  With j = 0 no H is kept.
 * 5. Emit.  linear_rgb = D * albedo on the channels step 0 divided, D elsewhere; accumulated_rgb is A treated likewise; rgba8 is linear_rgb after
 *    main.rs:219-225 with alpha 255; variance_rgb = var and filtered_variance_rgb = Dv, both in the filter's units (of c, not of C);
 *    length, prev_xy as TV's; moment1_rgb = M1, moment2_rgb = M2, history_rgb = H (M1 with j = 0): the state the next call reprojects, in the
 *    filter's units; raw_rgb, albedo, normal, depth, alpha: C and F as the call took or rendered them; image_ms: device time of steps 0 - 5.
 * rttnw_svgf_frame is rttnw_svgf_push of rttnw_render's out_linear_rgb and of rttnw_render_features' maps taken with spp = feature_spp (0:
 *   min(p->spp, 16)) and the same sample_begin; raw_rgb and the four maps are those calls' outputs, bit for bit.  p->width and p->height must equal
 *   the handle's, p->tile_world must be 1, the scene's device must be the handle's; the caller chooses p->sample_begin per frame.  stats
 *   (optional) is rttnw_render's, its `samples` and `rays` increased by the w * h * feature_spp camera rays of the feature pass.
 * Arithmetic: the neighbours'.  Only + - * /, sqrt, floor, abs and comparisons; no product is fused into a sum; every sum in the order the composed
 *   contracts state; non-finite values are not special-cased.  The device code, a host build of the same headers (rttnw_amd/csrc/svgf.hpp and
 *   those it composes) and a restatement in numpy give the same bits, and they are the bits of the composition above made with the three entry points.
 * A known approximation.  With feedback, var is the variance of the raw running mean M1, not of the cleaner A: the moments are accumulated apart
 *   from the colour, as SVGF does.  The filter's colour stop is therefore conservative.
 * Refusals, before the device is touched, each message naming the call and the argument, RTTNW_ERR_INVALID: a NULL q, `out` handle pointer, cam or
 *   p; a NULL input array (the rttnw_svgf_out pointer itself may be NULL: the call then only advances the state); width * height == 0;
 *   everything rttnw_temporal_variance, rttnw_temporal_accumulate and rttnw_denoise refuse for t, v and d; feedback_iterations > d.iterations;
 *   demodulate > 1; reserved0 != 0; for rttnw_svgf_frame a size that differs from the handle's or tile_world != 1.
 * One call at a time per handle; handles are independent of each other.
 * Out of scope: a node-wide form; adaptive sampling inside the sequence; colour clamping of the history; the non-local-means and select filters
 *   as the spatial stage (non-local means and the regression filter now live below, at rttnw_svgf_set_regress; select stays out); the native rttnw
 *   program; moving geometry. */
typedef struct rttnw_svgf rttnw_svgf; /* opaque */
struct rttnw_svgf_params {
    uint32_t feedback_iterations; /* 0: the history is the unfiltered accumulation; j >= 1: the colour history is the filter's result after j
                                     passes (SVGF: 1); must be <= d.iterations */
    uint32_t demodulate;          /* 0 / 1: accumulate, estimate and filter colour / albedo; any other value refused */
    uint32_t feature_spp;         /* rttnw_svgf_frame only: samples of the feature pass; 0 = min(p->spp, 16) */
    uint32_t reserved0;           /* must be 0 */
    rttnw_temporal_params t;      /* each field as in its own entry point, 0 = its default */
    rttnw_variance_params v;
    rttnw_denoise_params d;
};
typedef struct rttnw_svgf_params rttnw_svgf_params;
struct rttnw_svgf_out { /* host arrays, each optional */
    double* linear_rgb;            /* w*h*3: the frame to show */
    uint8_t* rgba8;                /* w*h*4 */
    double* accumulated_rgb;       /* w*h*3: the filter's input, remodulated */
    double* variance_rgb;          /* w*h*3: the estimate handed to the filter, in the filter's units */
    double* filtered_variance_rgb; /* w*h*3: rttnw_denoise's out_variance_rgb, same units */
    double* length;                /* w*h, as rttnw_temporal_variance's out_length */
    double* prev_xy;               /* w*h*2, as its out_prev_xy */
    double* moment1_rgb;           /* w*h*3 each: the state the next call reprojects (filter's units) */
    double* moment2_rgb;
    double* history_rgb;
    double* raw_rgb;               /* w*h*3: the frame's colour before step 0 */
    double* albedo;                /* w*h*3, w*h*3, w*h, w*h: its features */
    double* normal;
    double* depth;
    double* alpha;
    double* image_ms;              /* one double: device time of everything behind the trace and the feature pass */
};
typedef struct rttnw_svgf_out rttnw_svgf_out;
int rttnw_svgf_create(uint32_t width, uint32_t height, const rttnw_svgf_params* q, rttnw_svgf** out);
void rttnw_svgf_destroy(rttnw_svgf* q);
int rttnw_svgf_reset(rttnw_svgf* q); /* drop the history: the next call is a first frame */
int rttnw_svgf_push(rttnw_svgf* q, const rttnw_camera_desc* cam, const double* linear_rgb, const double* albedo, const double* normal,
                    const double* depth, const double* alpha, const rttnw_svgf_out* out);
int rttnw_svgf_frame(rttnw_svgf* q, rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_svgf_out* out,
                     rttnw_stats* stats);

/* Clipping the reprojected history to the frame: rttnw_temporal_variance with neighbourhood variance clipping (Karis 2014; Salvi 2016) in front of
 * its blend.  The three blocks above leave colour clamping of the history out of their scope; clipping now lives here.  A history reprojected by
 * the first hit ghosts on glass, on mirrors and on anything that moves, depth and normal accept it there, and a ghost that lasts has a small
 * temporal variance: nothing above compares the history's colour with the frame it is blended into.  This call does: it takes the mean and the
 * standard deviation of THIS frame's colour over a small window and clips the reprojected history into mean +- gamma * sd before the blend.
 * Calling convention as rttnw_temporal_variance: every argument of that entry point in the same order, k after v, three optional outputs before
 * kernel_ms; host arrays in and out (row-major, top row first), blocking, on the current device, no scene handle; no CPU fallback:
 * RTTNW_ERR_HIP without a device.  Everything is double.
 *
 * Stage S, the frame's statistics.  pos(x) = x < 0 ? 0 : x.  For a pixel with alpha != 0: the window of rttnw_temporal_variance's spatial
 *   estimate — dy = -radius .. radius (outer), dx = -radius .. radius (inner), the centre among the taps; taps outside the image, or whose
 *   alpha == 0, are dropped; a tap weighs w = w_n * w_z in that stage's expressions — with radius and sigmas from k, over the planes m1' = cur (this
 *   frame's colour) and m2' = cur * cur (rounded once).  Sw = sum w;  Sw > 0: mu = (sum w * m1') / Sw and q = (sum w * m2') / Sw;  otherwise
 *   mu = cur and q = cur * cur.  sd = sqrt(pos(q - mu * mu)).  A pixel with alpha == 0 has mu = cur, sd = 0.  lo = mu - gamma * sd;
 *   hi = mu + gamma * sd: one product and one sum each, not fused.  out_mean_rgb = mu and out_sd_rgb = sd, for every pixel.
 * Stage A', accumulate.  rttnw_temporal_variance's stage A in its expressions and its order up to the history's means h1 = (sum wt * m1') / W and
 *   h2 = (sum wt * m2') / W.  Then per channel h1c = h1 < lo ? lo : (h1 > hi ? hi : h1).  Every comparison with a NaN is false, so a NaN history,
 *   NaN bounds, or the inf * 0 bounds of gamma = +inf with sd = 0 clip nothing.  Bit ch of out_clipped is set exactly where one of the two
 *   branches was taken.  On a clipped channel h2c = (h2 - h1 * h1) + h1c * h1c: the history keeps its spread about the moved mean; on an unclipped
 *   channel h2c = h2 — a branch, not arithmetic.  The blend is stage A's with h1c and h2c in place of h1 and h2: out = (1 - a) * h1c + a * cur,
 *   out_m2 = (1 - a) * h2c + a * s.  out_length, out_prev_xy and every pass-through case (no history, alpha == 0, no place in the previous frame,
 *   W > 0 false) are stage A's, with out_clipped = 0.
 * Stage B, estimate.  rttnw_temporal_variance's, unchanged, on stage A''s outputs; its window takes radius and sigmas from v.
 * Consequences.  Where no channel of a pixel is clipped, every shared output equals rttnw_temporal_variance's bits there (out_variance_rgb on the
 *   spatial branch: where no pixel of its window was clipped).  With gamma = +inf every shared output equals rttnw_temporal_variance's bits and
 *   out_clipped is all 0.
 * Arithmetic.  + - * /, sqrt, floor, abs and comparisons only; every sum starts from 0.0 and adds in the order stated; no product is fused into a
 *   sum; non-finite values are not special-cased.  So the device code, a host build of the same header (rttnw_amd/csrc/clamp.hpp) and a
 *   restatement in numpy give the same bits.
 * Outputs, each optional: rttnw_temporal_variance's six; out_mean_rgb w*h*3; out_sd_rgb w*h*3; out_clipped w*h bytes; kernel_ms: device time of
 *   both kernels (the fused statistics-and-accumulate kernel, the estimate).
 * Refusals, before the device is touched, each message naming temporal_clamp and the argument, RTTNW_ERR_INVALID: everything
 *   rttnw_temporal_variance refuses, in its order; then a NULL k, k->radius > 4, k->reserved0 != 0, a negative or NaN gamma, a negative or NaN
 *   sigma.
 * The handle.  rttnw_svgf_set_clamp switches clipping on for an rttnw_svgf handle (NULL: off, the default); it takes effect from the next frame
 *   call, keeps the history, refuses what rttnw_temporal_clamp refuses for k (the handle is checked last), and allocates the one byte map it needs:
 *   frame calls still allocate nothing (the kernel's tile fits the LDS a kernel has without asking).  With a clamp set two steps of the handle's
 *   contract change, everything else stays:
 *   1. TV = rttnw_temporal_clamp(...) over the same arguments, k beside them.
 *   2. With feedback and a state, A = rttnw_temporal_clamp(cam, cam', c, F, prev_linear_rgb = H, prev_moment2_rgb = M2, prev_length = L, the state's
 *      normal, depth and alpha, t, v, k).out_linear_rgb.  The bounds depend only on c, F and k, so H is clipped to the same interval as M1.
 *   rttnw_svgf_clipped copies out the last frame call's map, w*h bytes: bits 0 - 2 are TV's out_clipped, bits 4 - 6 the H call's (0 without
 *   feedback); before any frame call, or after a call without a clamp, the map is all 0.  With `demodulate` the statistics are those of c, so a
 *   texture does not widen the interval.  With gamma = +inf every field of rttnw_svgf_out equals the unclamped handle's bits.
 * Out of scope: clipping in another colour space (YCoCg); cutting the history length where a pixel was clipped; a "fast history" as the source of
 *   the bounds; a node-wide form; the native rttnw program. */
struct rttnw_clamp_params {
    uint32_t radius;     /* the window is (2 radius + 1)^2; 0 = default 3; 1 .. 4 */
    uint32_t reserved0;  /* must be 0 */
    double gamma;        /* half-width of the admitted interval in standard deviations; 0 = default 1.0; +inf = never clip;
                            negative or NaN refused */
    double sigma_normal, sigma_depth; /* as rttnw_variance_params: 0 = rttnw_denoise's defaults */
};
typedef struct rttnw_clamp_params rttnw_clamp_params;
int rttnw_temporal_clamp(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam,
                         const double* linear_rgb, const double* normal, const double* depth, const double* alpha,
                         const double* prev_linear_rgb, const double* prev_moment2_rgb, const double* prev_length,
                         const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                         const rttnw_temporal_params* t, const rttnw_variance_params* v, const rttnw_clamp_params* k,
                         double* out_linear_rgb, uint8_t* out_rgba8, double* out_moment2_rgb, double* out_length, double* out_prev_xy,
                         double* out_variance_rgb, double* out_mean_rgb, double* out_sd_rgb, uint8_t* out_clipped, double* kernel_ms);
int rttnw_svgf_set_clamp(rttnw_svgf* q, const rttnw_clamp_params* k);   /* NULL: off, the default */
int rttnw_svgf_clipped(rttnw_svgf* q, uint8_t* out_clipped);            /* w*h: the last frame call's map */

/* Adaptive sampling inside the SVGF sequence: pixels whose history is thin get more samples in this frame.  The handle's block above leaves
 * adaptive sampling inside the sequence out of its scope; it now lives here.  Along an orbit a large share of the pixels finds no history (a
 * disocclusion, the frame's edge) and enters the filter with the frame's few samples beside neighbours that hold dozens of frames.  Which pixels
 * those are is known BEFORE the trace: reprojection needs this frame's first-hit features and the state's, not its colour.
 *
 * rttnw_temporal_probe: where each pixel's history is, and how long, without colour.  Calling convention as rttnw_temporal_accumulate: host arrays
 * in and out (row-major, top row first), blocking, on the current device, no scene handle; no CPU fallback: RTTNW_ERR_HIP without a device.
 * Everything is double.
 * Pixel rule.  rttnw_temporal_accumulate's geometry and acceptance, unchanged: steps 1 and 2 of that contract (the surface point, its place
 *   (fx, fy) in the previous frame and its distance zq there), then the four taps in the order 00, 10, 01, 11 through that contract's tests,
 *   with the same wt, sw = sw + wt and sl = sl + wt * prev_length[tp].  Where sw > 0, Lp = sl / sw.  Lp = 0.0 on every pass-through case: no
 *   history, alpha == 0, no place in the previous frame, or sw > 0 false.  out_length = Lp.  out_prev_xy is rttnw_temporal_accumulate's.
 * Multiplier.  k = floor(fill / (Lp + 1.0)).  m is the largest of 1, 2, 4, 8 that is <= min(k, boost); m = 1 when k < 1 (a NaN compares false:
 *   m = 1), and m = 1 where this frame's alpha == 0.  out_multiplier = m, one byte a pixel.
 * Consequence.  With the same inputs rttnw_temporal_accumulate's out_length equals Lp == 0 ? 1 : min(Lp + 1, max_history), bit for bit (min as
 *   that contract takes it: grown < max_history ? grown : max_history), and the two out_prev_xy are equal bitwise, NaNs included.
 * Arithmetic.  + - * /, sqrt, floor and comparisons only; no product is fused into a sum; every sum starts from 0.0 and adds in the order
 *   stated; non-finite values are not special-cased.  So the device code, a host build of the same header (rttnw_amd/csrc/probe.hpp) and a
 *   restatement in numpy give the same bits.
 * Outputs, each optional: out_length w*h; out_prev_xy w*h*2; out_multiplier w*h bytes; kernel_ms: device time of the one kernel.
 * Refusals, before the device is touched, each message naming temporal_probe and the argument, RTTNW_ERR_INVALID: everything
 *   rttnw_temporal_accumulate refuses for the arguments the two calls share, in its order (a NULL cam; a NULL normal, depth or alpha; a NULL t; an
 *   empty image or more than 2^28 pixels; the four prev_* arrays not all or none; a history without prev_cam; t's fields); then a NULL a, a->boost
 *   not in {0, 1, 2, 4, 8}, a->reserved0 != 0, and a->fill that is NaN, infinite or in (0, 1).
 *
 * The handle.  rttnw_svgf_set_sampling switches sampling on for an rttnw_svgf handle (NULL: off, the default); it takes effect from the next frame
 *   call, keeps the history, refuses what rttnw_temporal_probe refuses for a (the handle is checked last), and allocates what it needs there and
 *   then (two maps, the mask and selection bytes, the list of 2x2 blocks and the list passes' sums: 44 bytes a pixel).  rttnw_svgf_push is
 *   unaffected: the caller rendered that frame.  rttnw_svgf_out and rttnw_svgf_params are unchanged.  With sampling set, rttnw_svgf_frame changes in
 *   one place, the colour C it renders:
 *   1. The feature pass runs first; it does not depend on the trace, so F keeps its bits.
 *   2. m = rttnw_temporal_probe(cam, cam', F, the state's L, normal, depth and alpha, t, a).out_multiplier.  With an empty state
 *      m = min(boost, largest power of two <= floor(fill)) on every hit pixel, 1 on every miss.
 *   3. For every pixel, C(p) is the pixel of rttnw_render(s, cam, p with spp = m(p) * p->spp, the same sample_begin), bit for bit; equivalently
 *      of rttnw_render_region under the mask {m == level} with spp = level * p->spp.
 *   4. Steps 0 to 5 of the handle's contract run on that C, unchanged, also with a clamp set.
 *   So a frame call with sampling equals rttnw_svgf_push of that composed C and of F, in every output.  With boost = 1, or sampling never set,
 *   every output and the handle's state are the bits of a handle without it.
 * How it is traced.  Everything stays on the device.  The plain pass traces EVERY pixel at p->spp as without sampling; then, per level 2, 4, 8 up
 *   to boost, the pixels of that level are listed as rttnw_render_region lists a mask, traced at level * p->spp, and written over the plain
 *   pass's.  The plain pass's samples of a boosted pixel are discarded.  Each level's list reads its length back with an 8-byte copy, so the call
 *   waits up to three more times than without sampling; a level nobody holds traces nothing.
 * Accounting.  stats->samples counts what was traced, the discarded samples included: width * height * p->spp of the plain pass, plus
 *   m(p) * p->spp of every pixel with m(p) > 1, plus the feature pass's rays as without sampling.  stats->rays is what it is without sampling (the
 *   feature pass's rays: the handle takes no counters).  stats->kernel_ms is the plain pass's plus the time from the probe to the last level's
 *   write, the waits for the lists' lengths included.
 *   rttnw_svgf_samples copies out the last rttnw_svgf_frame call's map, each array optional: out_spp w*h, m(p) * p->spp; out_length w*h, Lp.
 *   Before any frame call out_spp is all 0 and out_length all 0; after a frame call without sampling out_spp is that call's p->spp everywhere and
 *   out_length all 0.  rttnw_svgf_push leaves the map as it is.
 * Sample indices.  A frame call with sampling may consume sample indices [sample_begin, sample_begin + boost * spp): a caller who wants
 *   independent frames advances p->sample_begin by boost * p->spp a frame.  rttnw_svgf_frame refuses, before the device is touched and on the terms
 *   of its other checks (RTTNW_ERR_INVALID, naming svgf_frame), a p->spp whose product with the handle's boost is no spp rttnw_render accepts
 *   (more than 2^32 - 1).
 * Deliberately unchanged: the blend still weighs a frame as one frame, whatever its sample count.  With the defaults (boost 8, fill 8.0) a
 *   disoccluded pixel gets 8, 4, 2, 2, 1, ... times spp over its first frames (Lp = 0, 1, 2, 3, 4): the schedule decays instead of stepping.
 * Out of scope: a sample-weighted history length; dilating the multiplier map; a different rule for the first frame; the variance, not only the
 *   length, as the driver; a node-wide form; the native rttnw program. */
struct rttnw_sampling_params {
    uint32_t boost;      /* largest multiplier of p->spp a pixel may get: 1, 2, 4 or 8; 0 = default 8 */
    uint32_t reserved0;  /* must be 0 */
    double fill;         /* a pixel is boosted while (reprojected length + 1) * m <= fill; 0 = default 8.0; >= 1, finite */
};
typedef struct rttnw_sampling_params rttnw_sampling_params;
int rttnw_temporal_probe(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam,
                         const double* normal, const double* depth, const double* alpha,
                         const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                         const rttnw_temporal_params* t, const rttnw_sampling_params* a,
                         double* out_length, double* out_prev_xy, uint8_t* out_multiplier, double* kernel_ms);
int rttnw_svgf_set_sampling(rttnw_svgf* q, const rttnw_sampling_params* a);  /* NULL: off, the default */
int rttnw_svgf_samples(rttnw_svgf* q, uint32_t* out_spp, double* out_length); /* w*h each, optional: the last rttnw_svgf_frame call's map */

/* The regression filter as the SVGF spatial stage: the handle carries two half-buffer histories along its reprojection and hands them, with its
 * temporal variance estimate, to rttnw_denoise_regress.  The handle's block above leaves the non-local-means filter as the spatial stage out of its
 * scope, and rttnw_denoise_regress's leaves out the SVGF handle; both now live here.  rttnw_denoise leans on the first hit alone and blurs what it
 * does not describe — a noise texture, what mirrors and glass show; rttnw_denoise_nlm and rttnw_denoise_regress measure their weights on the colour,
 * but on a single frame they measure them on two halves of a few samples each.  Here the weights are measured on ACCUMULATED halves.  With
 * g->features == 0 the same switch gives non-local means as the spatial stage.  No new struct: rttnw_svgf_params and rttnw_svgf_out are unchanged.
 *
 * rttnw_svgf_set_regress switches the stage on for an rttnw_svgf handle (g NULL: off, the default); variance_source chooses the variances the
 *   filter's weights read: 0 the handle's temporal estimate, 1 the filter's own pair variance.  Setting or clearing the stage resets the history,
 *   as rttnw_svgf_reset does (a history without the halves is none); a NULL g on a handle without the stage is a no-op and keeps the history.
 *   Every buffer the stage needs is allocated there and then and the filter kernel's dynamic LDS is admitted — a second packed trace buffer, the
 *   two ingested halves, Ha and Hb as ping-pong pairs, and the filter's workspace (records, the two filtered halves, fit bytes, error, fit): frame
 *   calls still allocate nothing.  The stage is exclusive with feedback_iterations != 0, a clamp and sampling.
 * The contract is a composition of the existing entry points, bit for bit.  With the stage set the state gains Ha and Hb, the accumulated halves;
 *   the rest of the state is unchanged.  A call has the halves a and b, features F and camera cam; cam' is the state's camera.
 *   C = (a + b) * 0.5: this is raw_rgb.
 * 0. The handle's step 0 applied to C, a and b separately, giving c, ca, cb; the "was divided" channels are C's (the rule reads F only).
 * 1. The handle's step 1 on c, unchanged: TV = rttnw_temporal_variance(...) gives M1, M2, L, prev_xy and var.  Consequence: these five, and
 *    moment1_rgb, moment2_rgb, length, prev_xy and variance_rgb, equal bit for bit those of a plain handle (feedback 0, the same t, v and demodulate)
 *    pushed with C.
 * 2. With a state, Aa = rttnw_temporal_accumulate(cam, cam', ca, no variances, F, prev_linear_rgb = Ha, prev_length = L, the state's normal, depth
 *    and alpha, t).out_linear_rgb, and Ab likewise from cb over Hb; on the device the four taps are computed once and carry four quantities.  Without
 *    a state Aa = ca and Ab = cb.  The new Ha and Hb are Aa and Ab: there is no feedback.
 * 3. R = rttnw_denoise_regress(Aa, Ab, var_a, var_b, F.albedo, F.normal, F.depth, F.alpha, g).  variance_source 0: var_a = var_b = var + var, one
 *    sum — each half is a mean over half the samples of M1, so its variance is twice M1's.  variance_source 1: both NULL, the filter's own pair
 *    variance.  g->demodulate must be 0: the handle's demodulate does that job.  F.albedo is passed as a regressor, not as a divisor, also when the
 *    handle demodulates.  With g->features == 0 this step is rttnw_denoise_nlm(Aa, Ab, var_a, var_b) bit for bit (property 1 of that contract).
 * 5. Emit.  linear_rgb = R.out_linear_rgb multiplied back on the channels step 0 divided, rgba8 made from it; accumulated_rgb = (Aa + Ab) * 0.5
 *    treated likewise; filtered_variance_rgb = R.out_error_rgb; history_rgb = M1; everything else as without the stage.
 * rttnw_svgf_push_halves is rttnw_svgf_push for a handle with the stage: half_a and half_b (w*h*3 each) stand where linear_rgb stood.
 * rttnw_svgf_frame on such a handle renders Ca = rttnw_render(spp = p->spp / 2, sample_begin) and Cb = rttnw_render(spp = p->spp / 2,
 *   sample_begin + p->spp / 2), the feature pass as without the stage, and is then rttnw_svgf_push_halves of those, bit for bit in every
 *   precision.  p->spp must be even and at least 2.  stats sums the two traces.
 * rttnw_svgf_halves copies out, each array optional, Aa, Ab, R.out_half_a and R.out_half_b (w*h*3 each) and R.out_fit (w*h) of the last frame call,
 *   in the filter's units; before any frame call with the stage — and after the stage was set anew or cleared — every array is all 0.
 * Refusals, before the device is touched, each message naming the call, RTTNW_ERR_INVALID.  rttnw_svgf_set_regress, in this order: everything
 *   rttnw_denoise_regress refuses for g, in its order; g->demodulate != 0; variance_source > 1; a NULL q (the handle is checked last); a handle with
 *   feedback_iterations != 0, a clamp set or sampling set.  rttnw_svgf_set_clamp and rttnw_svgf_set_sampling with a non-NULL block refuse a handle
 *   with the stage; rttnw_svgf_push refuses one; rttnw_svgf_push_halves refuses a handle without it, after rttnw_svgf_push's own checks;
 *   rttnw_svgf_frame on a handle with the stage refuses an odd p->spp and p->spp < 2.
 * Out of scope: rttnw_denoise_select as a stage; feeding the filtered halves back into Ha and Hb; a clamp or sampling together with this stage; a
 *   sample-weighted blend; a node-wide form; the native rttnw program. */
int rttnw_svgf_set_regress(rttnw_svgf* q, const rttnw_regress_params* g, uint32_t variance_source); /* g NULL: off, the default */
int rttnw_svgf_push_halves(rttnw_svgf* q, const rttnw_camera_desc* cam, const double* half_a, const double* half_b,
                           const double* albedo, const double* normal, const double* depth, const double* alpha,
                           const rttnw_svgf_out* out);
int rttnw_svgf_halves(rttnw_svgf* q, double* out_acc_a, double* out_acc_b, double* out_filtered_a, double* out_filtered_b,
                      double* out_fit); /* w*h*3 x4, w*h; each optional; the last frame call's, in the filter's units */

/* `render()` on the GPUs of ONE NODE, in one call from one host thread ("library owns its HIP
 * streams / RCCL comms"): the framebuffer's 8x8 tiles are interleaved over `ngpu` ranks, rank r traces its tiles on
 * device `device_ids[r]` (the scene is replicated there on first use), the packed tiles are gathered on rank 0's device —
 * grouped ncclSend/ncclRecv over xGMI between different devices (RCCL is loaded at the first call that needs it), a
 * device-to-device copy for ranks that share rank 0's device — and un-tiled there.  A device may appear more than once
 * (logical ranks; they run one after the other on it), so any partition can be exercised on a single GPU.  The image is
 * bit-identical to rttnw_render's for every ngpu.  Outputs as rttnw_render; `p->tile_rank` / `p->tile_world` are ignored;
 * `stats` (optional) points to ngpu records: samples and device time (trace + resolve) of each rank.  Blocking.
 * Environment: RTTNW_MULTI_GATHER=rccl (default) | peer — `peer` gathers with hipMemcpyPeerAsync on each rank's stream (an event orders
 * the root's un-tile behind it) instead of RCCL; the call falls through to it by itself, with one line on stderr, when RCCL cannot be loaded
 * or ncclCommInitAll fails (stats[0].reserved bits 8 / 9). */
int rttnw_render_multi(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint32_t ngpu,
                       const int32_t* device_ids, double* out_linear_rgb, uint8_t* out_rgba8, rttnw_stats* stats);

/* Adaptive sampling on the GPUs of ONE NODE: rttnw_render_adaptive over the ranks of rttnw_render_multi, in one call from one host thread.
 * (Came without a version bump, like rttnw_render_adaptive: detect it by its symbol.)
 *
 * Contract.  The four outputs — linear image, RGBA8, samples map, standard-error map (the +inf of a pixel with fewer than two chunks included) —
 *   are BIT-IDENTICAL to rttnw_render_adaptive(s, cam, p, a, ...): for every ngpu, every device list (a device may repeat: logical ranks, as in
 *   rttnw_render_multi), both gather transports and the fall-through between them, every `precision`, every kernel form and every launch split
 *   (RTTNW_CHUNK_SUM_BUDGET).  A pixel's stopping decision reads its own chunk sums only, so it does not matter which rank traces it.
 * Ranks.  Rank r owns the tiles rttnw_render_multi gives it, on device device_ids[r].  Pass 0 traces them in the plain render's job numbering;
 *   pass k > 0 traces the list of the rank's 2x2 blocks that still hold an active pixel.  Every pass is enqueued on all ranks that still have
 *   active pixels before the host waits for any of them (ranks that share a device run one after the other on it); a rank whose list is empty
 *   takes no further part.  `p->tile_rank` / `p->tile_world` are ignored, as in rttnw_render_multi.
 * Gather.  Each rank's packed means and a second buffer of the same shape — standard error r, g, b and the sample count, 4 doubles per pixel —
 *   reach rank 0's device by rttnw_render_multi's transports, under its environment (RTTNW_MULTI_GATHER), and are un-tiled there.
 * Outputs as rttnw_render_adaptive (each optional).  `stats` (optional) points to ngpu records: stats[r].samples = the samples rank r traced
 *   (their sum over r is the single call's stats.samples), kernel_ms = device time of all of rank r's passes, list building included, reserved =
 *   the kernel form (rank 0 also carries bits 8 and 9, as in rttnw_render_multi), and the scene's sizes as usual.  Blocking.
 * Refusals, before the device is touched, in this order: RTTNW_ERR_INVALID for a NULL p or a, ngpu == 0, ngpu > 64 or a NULL device_ids; what
 *   rttnw_render_adaptive refuses among its own arguments, with its codes (pass_spp == 0, p->spp not a positive multiple of pass_spp, a negative
 *   or NaN tolerance, a->reserved0 != 0: RTTNW_ERR_INVALID; collect_counters != 0: RTTNW_ERR_UNSUPPORTED) except its tile_world rule; whatever
 *   rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes); RTTNW_ERR_INVALID for a device id outside
 *   [0, rttnw_device_count()). */
int rttnw_render_adaptive_multi(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                                uint32_t ngpu, const int32_t* device_ids,
                                double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb,
                                rttnw_stats* stats);

/* An adaptive render that can be taken up again: rttnw_render_adaptive / rttnw_render_adaptive_multi begun from, and left as, a STATE — a preview at
 * 5 % noise refined to 2 %, a cap that turned out too low raised, a long render that survives its process — without retracing a sample.
 * (Came without a version bump, like rttnw_render_adaptive: detect it by its symbol.)
 *
 * The state is a host array of rttnw_adaptive_state_doubles(width, height) = 64 + 12 * width * height doubles; every integer in it is exact.
 *   Header, doubles [0, 64), unused entries 0:
 *     [0] RTTNW_ADAPTIVE_STATE_MAGIC   [1] RTTNW_ADAPTIVE_STATE_VERSION   [2] width   [3] height   [4] a->pass_spp
 *     [5] p->spp_chunk as the caller passed it (0 allowed)   [6] sample_begin   [7] precision   [8] max_depth   [9] quirks
 *     [10], [11] the low and the high 32 bits of seed   [12] t_min   [13..15] background   [16..30] the 15 doubles of rttnw_camera_desc, in field order
 *   Per pixel, 12 doubles, row-major, top row first, the pixels of the image only:
 *     [0..2] sum r, g, b   the running chunk-sum chain in the kernel's arithmetic type, widened to double (exact for RTTNW_F32: it narrows back exactly)
 *     [3]    n             samples folded (n_q)
 *     [4..6] mu r, g, b    the weighted mean of the chunk means (rttnw_render_adaptive's "Noise estimate")
 *     [7]    k             chunks folded: (n / B) * the chunks of a pass of B samples under spp_chunk (spp_chunk c != 0: ceil(B / c); 0, the default
 *                          schedule: with tail = B below 32 ? B : B / 32 and main = (B - tail) / 4, main + (B - 4 main) — B = 32: 11, B = 16: 16)
 *     [8..10] m2 r, g, b   M2 = sum_c n_c (m_c - mu)^2
 *     [11]   0
 *   The state holds neither the tolerances nor the cap: those may change from call to call.  It does NOT identify the scene — nothing in it is
 *   derived from the scene — so the caller resumes on the scene it started on; resuming on another is not detected and renders a mixture.
 * Where it runs.  ngpu == 0 with device_ids == NULL: the scene's device, as rttnw_render_adaptive (`stats`: one record; tile_world must be 1).
 *   ngpu 1 .. 64: rttnw_render_adaptive_multi's ranks, gather transports and environment (`stats`: ngpu records; tile_rank / tile_world ignored).
 * state_in == NULL.  The four outputs and `stats` are rttnw_render_adaptive's (ngpu == 0) or rttnw_render_adaptive_multi's, BIT FOR BIT, and the state
 *   the render ends in is written to state_out (optional).
 * state_in != NULL.  Every pixel q starts from its record: sum, noise state and n_q samples.  Its active bit is decided anew under THIS call's
 *   tolerances and cap, by the expression that ends a pass (value = sum / n_q in the kernel's type, then the stopping rule).  Passes go by LEVEL:
 *   level k traces samples [sample_begin + kB, sample_begin + (k+1)B) of the pixels that are active and have n_q == kB, over the list of their 2x2
 *   blocks — the jobs rttnw_render(spp = B, sample_begin = sample_begin + kB) runs for them.  Levels run from the lowest n_q / B of the state to
 *   spp / B - 1; a level nobody stands at costs its list build and is skipped, and the loop ends once no pixel is active at any level.  In the
 *   node-wide form every rank works at the same level, each level enqueued on all live ranks before the host waits for any.
 * Contract.  Let S be the state of a run with cap C1 and tolerances (rel1, abs1).  Resumed with a cap C2 >= C1 and tolerances rel2 <= rel1,
 *   abs2 <= abs1, the four outputs and state_out are BIT-IDENTICAL to those of ONE call with state_in == NULL, cap C2 and (rel2, abs2) — for every
 *   `precision`, every kernel form, every launch split (RTTNW_CHUNK_SUM_BUDGET), every ngpu and device list on either side of the hand-over (the
 *   state is row-major: begun on one GPU it continues on eight, and the reverse) and both gather transports.  Why: a pixel's samples are keyed by
 *   (pixel, sample, seed), its sum is one chain in chunk order and its stopping decision reads its own chunk sums only; a tighter rule and a
 *   higher cap can only stop a pixel LATER, so no pixel of S holds more samples than the uninterrupted run would have given it, and the passes
 *   that remain are the ones that run had left.  With a LOOSER tolerance or a lower cap than the state was made under the call is still well
 *   defined — a pixel keeps what it has and goes on only if it is active — but no longer equal to a fresh render: pixels may hold more samples
 *   than the looser rule would have given them.
 * No work.  When no pixel is active: RTTNW_OK, no trace kernel is launched, stats->samples == 0, the outputs are those of the state's own run.
 * Outputs as rttnw_render_adaptive (each optional), and state_out (optional; state_in and state_out may be the SAME array).  `stats` (optional):
 *   samples = what THIS call traced, not the state's (node-wide: per rank; over the ranks it is sum(out_spp) minus the state's n summed),
 *   kernel_ms = device time of everything the call runs, the state's copy to the device and its conversion both ways included; reserved and the
 *   scene's sizes as for rttnw_render_adaptive.  Apart from the state's copies and the one 8-byte copy per pass, no host round trip.  Blocking.
 * Refusals, before the device is touched, in this order, each message naming render_adaptive_resume and the field:
 *   1. RTTNW_ERR_INVALID for a NULL p or a;
 *   2. RTTNW_ERR_INVALID for ngpu > 64, ngpu >= 1 with a NULL device_ids, ngpu == 0 with a non-NULL device_ids;
 *   3. what rttnw_render_adaptive refuses among its own arguments, with its codes (its tile_world rule with ngpu == 0 only);
 *   4. with a state_in, RTTNW_ERR_INVALID for a wrong magic number or version; for a header field that differs — compared bitwise — from this
 *      call's: width, height, pass_spp, spp_chunk, sample_begin, precision, max_depth, quirks, seed, t_min, background, the camera's 15 doubles;
 *      and (unless width or height is 0: the records are then not looked at) for a record whose n or k is not a finite integer, n < B, n not a
 *      multiple of B, n > p->spp ("the state holds more samples than the cap"), or k != (n / B) * the chunks of a pass;
 *   5. whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes);
 *   6. with ngpu >= 1, RTTNW_ERR_INVALID for a device id outside [0, rttnw_device_count()). */
#define RTTNW_ADAPTIVE_STATE_MAGIC 1381256791u /* 0x52544E57, "RTNW" */
#define RTTNW_ADAPTIVE_STATE_VERSION 1u
#define RTTNW_ADAPTIVE_STATE_HEADER 64u /* doubles before the first record */
#define RTTNW_ADAPTIVE_STATE_RECORD 12u /* doubles per pixel */
uint64_t rttnw_adaptive_state_doubles(uint32_t width, uint32_t height);
int rttnw_render_adaptive_resume(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                                 uint32_t ngpu, const int32_t* device_ids, const double* state_in, double* state_out,
                                 double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb,
                                 rttnw_stats* stats);

/* Adaptive sampling of a window, or a pixel mask, of the frame: rttnw_render_adaptive_resume over the selection of rttnw_render_region — a preview of
 * the area being worked on sampled to a noise target, the noisy patch of an adaptive preview brought to 2 % where one looks — at the cost of the
 * selected pixels' samples.  (Came without a version bump, like rttnw_render_adaptive: detect it by its symbol.)
 *
 * Frame, window, mask.  As rttnw_render_region: the frame is the p->width x p->height frame of rttnw_render, with its camera and its keys (pixel,
 *   sample, seed); the window is its pixels [x0, x1) x [y0, y1), row 0 = top; `mask` (optional): (x1-x0)*(y1-y0) bytes, row-major, top row first,
 *   nonzero = selected; NULL selects every pixel of the window.  Selected pixels are the only ones this call may trace.
 * Where it runs.  As rttnw_render_adaptive_resume: ngpu == 0 with device_ids == NULL on the scene's device (`stats`: one record; tile_world must
 *   be 1); ngpu 1 .. 64 on rttnw_render_adaptive_multi's ranks, with its gather transports and environment (`stats`: ngpu records).
 * State.  The state of rttnw_render_adaptive_resume: same magic, version, header and size rttnw_adaptive_state_doubles(width, height) — always
 *   FRAME-sized and row-major, whatever the window.  One addition, for this entry point only: a record of twelve zeros means "this pixel holds no
 *   samples yet".  state_in == NULL stands for a state whose records are all zero.  rttnw_render_adaptive_resume keeps refusing such records (n
 *   below pass_spp); a partly filled state is completed by a call of this entry point over the whole frame, after which resume accepts it.
 * What is traced.  Every pixel starts from its record.  A selected pixel with a zero record is active; a selected pixel with samples is active
 *   by the expression that ends a pass (value = sum / n_q in the kernel's type, then the stopping rule) under THIS call's tolerances and cap; an
 *   unselected pixel is never active, and its record goes to state_out unchanged, bit for bit.  Passes go by LEVEL, as in the resumed render:
 *   level k traces samples [sample_begin + kB, sample_begin + (k+1)B) of the active pixels that hold exactly kB samples, over the list of their 2x2
 *   blocks — level 0 too runs over a list, not in the plain render's job numbering.  Levels run from the lowest a selected pixel stands at to
 *   spp / B - 1; a level nobody is active at costs its list build, and the loop ends once no pixel is active.
 * Outputs (each optional, sized by the WINDOW; row-major, top row first): out_linear_rgb (x1-x0)*(y1-y0)*3 doubles, out_rgba8 *4 bytes, out_spp
 *   *1 words, out_stderr_rgb *3 doubles.  They report every pixel of the window that holds samples in the state the call ends in, selected or not:
 *   its mean (sum / n_q in the kernel's type, the adaptive render's division), RGBA8 with alpha 255, n_q, and its standard error (+inf with fewer
 *   than two chunks).  A pixel of the window without samples gets 0, 0, 0, RGBA8 0, 0, 0, 0, spp 0 and stderr 0: alpha tells the two apart, as
 *   in rttnw_render_region.  state_out (optional; may be the SAME array as state_in): the header, then every record of the frame.
 * Contract.  Let F be the four outputs and the state of ONE rttnw_render_adaptive_resume(state_in = NULL) of the frame with cap C and tolerances
 *   (rel, abs), and q a pixel this call selected and ended under cap C and (rel, abs), every earlier call that traced q having used a cap no higher
 *   and tolerances no tighter.  Then q's record in state_out, its linear value, RGBA8, sample count and standard error are BIT-IDENTICAL to q's
 *   in F — for every `precision`, every kernel form, every launch split (RTTNW_CHUNK_SUM_BUDGET), every ngpu and device list on either side of any
 *   hand-over, and both gather transports.  Why: the resumable form's reason — a pixel's samples are keyed by (pixel, sample, seed), its sum is one
 *   chain in chunk order (0 + c0 is that chain's first addition, so a list pass on a zero record is the plain pass 0), and its stopping decision
 *   reads its own chunk sums only.  With a LOOSER rule than q was last traced under the call is still well defined — a pixel keeps what it has and
 *   goes on only if it is active — but no longer equal to a fresh render: q may hold more samples than the looser rule would have given it.
 * No work.  Nothing active (an all-zero mask, or every selected pixel done): RTTNW_OK, no trace kernel is launched, stats->samples == 0, and the
 *   outputs are those of the incoming state — with no state and an all-zero mask all cleared, state_out a header over zero records.
 * `stats` (optional), as rttnw_render_adaptive_resume: samples = what THIS call traced (node-wide: per rank), kernel_ms = device time of
 *   everything the call runs, the state's copy to the device and its conversion both ways included; reserved and the scene's sizes as there.
 *   Blocking.
 * Memory.  The state, and per rank the packed means, noise state, active, selection and level bytes, the state records and the block list's
 *   workspace (a word per 2x2 block of the rank) are FRAME-sized, as in the resumable form.  Chunk sums are sized by the blocks that hold a
 *   selected pixel (4 per block and chunk), the mask and the four outputs by the window.  A window-sized state is out of scope.
 * Refusals, before the device is touched, in this order, each message naming render_adaptive_region and the field:
 *   1. RTTNW_ERR_INVALID for a NULL p or a;
 *   2. RTTNW_ERR_INVALID for x0 >= x1, y0 >= y1, x1 > width or y1 > height;
 *   3. RTTNW_ERR_INVALID for ngpu > 64, ngpu >= 1 with a NULL device_ids, ngpu == 0 with a non-NULL device_ids;
 *   4. what rttnw_render_adaptive refuses among its own arguments, with its codes (its tile_world rule with ngpu == 0 only);
 *   5. with a state_in, rttnw_render_adaptive_resume's state checks (the header compared bitwise; per record n and k finite integers, n a multiple
 *      of B, n <= p->spp, k == (n / B) * the chunks of a pass) with two differences: a record with n == 0 is accepted if and only if all twelve
 *      doubles are zero (RTTNW_ERR_INVALID for a zero n with anything else nonzero), and n < B is refused only for n != 0;
 *   6. whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes);
 *   7. with ngpu >= 1, RTTNW_ERR_INVALID for a device id outside [0, rttnw_device_count()). */
int rttnw_render_adaptive_region(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                                 uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const uint8_t* mask,
                                 uint32_t ngpu, const int32_t* device_ids, const double* state_in, double* state_out,
                                 double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb,
                                 rttnw_stats* stats);

/* Adaptive sampling for an image that will be FILTERED: the adaptive render and rttnw_denoise alternate on the device, and a pixel stops on the
 * standard error of the filtered image, not of its raw mean — smooth regions, where the filter averages many pixels, stop early; edges and
 * detail, where it cannot, keep sampling (Rousselle et al. 2012; the variance travels through the filter as in SVGF).  One GPU, tile_world == 1,
 * blocking.  (Came without a version bump, like rttnw_render_adaptive: detect it by its symbol.)
 *
 * Let B = a->pass_spp and the cap = p->spp, a positive multiple of B.
 * Before round 0.  The features F of the frame are rttnw_render_features' with p->spp replaced by g->feature_spp (0 means B) and p's
 *   sample_begin, seed and precision.  Every pixel is active.
 * Round k = 0 .. cap / B - 1, while any pixel is active:
 *   1. Trace.  Every active pixel gets samples [sample_begin + kB, sample_begin + (k+1)B): the jobs, chunk schedule, running-sum chain and
 *      noise-state update of rttnw_render_adaptive's passes, as a list pass over the 2x2 blocks that hold an active pixel (round 0 included).  All
 *      active pixels hold exactly kB samples, so a round is one level of rttnw_render_adaptive_resume's loop.
 *   2. Raw values of EVERY pixel of the frame, stopped ones with their frozen values: mean = sum / n_q in the kernel's type, widened to double;
 *      stderr as rttnw_render_adaptive defines it (+inf with fewer than two chunks); variance = stderr * stderr in double, not fused.
 *   3. Filter.  (den, var_f) = rttnw_denoise's out_linear_rgb and out_variance_rgb on (mean, variance, F, g->denoise), bit for bit.
 *   4. Stop.  An active pixel stops, for good, if its own stderr is 0 in r, g and b, or if for each of r, g, b var_f is finite and
 *          sqrt(var_f) <= abs_error + rel_error * den             (linear radiance, den = the filtered value)
 *      A stopped pixel is never reactivated.  Its decision depended on its neighbours' samples, so — unlike rttnw_render_adaptive — bit-identity
 *      with a fresh render at another tolerance or cap is NOT promised, and neither is a resume contract of rttnw_render_adaptive_resume's kind.
 * Outputs, of the last round that ran (each optional; row-major, top row first): out_linear_rgb w*h*3 the DENOISED image; out_rgba8 w*h*4 of
 *   the denoised image (main.rs:219-225); out_spp w*h the n_q; out_stderr_rgb w*h*3 sqrt of the FILTERED variance; out_raw_linear_rgb w*h*3 the
 *   unfiltered means (rttnw_render_adaptive's value); out_raw_stderr_rgb w*h*3 the unfiltered standard errors; state_out,
 *   rttnw_adaptive_state_doubles(w, h) doubles: the ordinary adaptive state, which rttnw_render_adaptive_resume and rttnw_render_adaptive_region
 *   accept.  `stats`: samples = sum_q n_q, kernel_ms = device time of everything the call runs, the feature pass and every denoise pass
 *   included, reserved = the kernel form, the scene's sizes as usual.
 * Contract.  The outputs are BIT-IDENTICAL to this host composition of entry points above, for every `precision`, kernel form and launch split
 *   (RTTNW_CHUNK_SUM_BUDGET).  With active_0 = every pixel, round k calls
 *     rttnw_render_adaptive_region(window = the whole frame, mask = active_k, ngpu = 0, cap (k+1)B, rel_error = abs_error = 0,
 *                                  state_in = round k-1's state_out, NULL in round 0),
 *     rttnw_denoise on that call's image and squared standard error, with F,
 *   and applies step 4.  (Under a tolerance of 0 the region call itself leaves a pixel with zero stderr untraced: step 4's first condition is
 *   what makes the two agree.)  With denoise.iterations == 0 the filter is the identity and out_spp, the raw and the filtered image, out_rgba8
 *   and out_raw_stderr_rgb are rttnw_render_adaptive's under the same cap, B and tolerances.
 * Where it lives.  Between rounds nothing frame-sized crosses to the host: per round the host reads 8 bytes, the length of the round's list and
 *   the number of active pixels.  The composition pays a state copy both ways (96 bytes per pixel) and the six uploads of rttnw_denoise per round.
 * Refusals, before the device is touched, in this order, each message naming render_adaptive_denoised and the field:
 *   1. RTTNW_ERR_INVALID for a NULL p, a or g;
 *   2. what rttnw_render_adaptive refuses among its own arguments, with its codes;
 *   3. RTTNW_ERR_INVALID for g->reserved0 != 0, g->denoise.iterations > 8, g->denoise.reserved0 != 0, a negative or NaN sigma;
 *   4. whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes).
 * Out of scope: a node-wide form (ngpu), a state_in, and windows or masks. */
struct rttnw_guided {
    uint32_t feature_spp;         /* samples per pixel of the feature buffers; 0 = a->pass_spp */
    uint32_t reserved0;           /* must be 0 */
    rttnw_denoise_params denoise; /* as rttnw_denoise: iterations 0 .. 8, sigmas (0 = the library default) */
};
typedef struct rttnw_guided rttnw_guided;
int rttnw_render_adaptive_denoised(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                                   const rttnw_guided* g, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp,
                                   double* out_stderr_rgb, double* out_raw_linear_rgb, double* out_raw_stderr_rgb, double* state_out,
                                   rttnw_stats* stats);

/* rttnw_denoise over an image of which only SOME pixels hold a value: a render of a mask or a lattice (rttnw_render_region,
 * rttnw_render_adaptive_region), a state that is still being refined.  rttnw_denoise treats every pixel as a value — a pixel that was never
 * sampled, linear 0, is averaged into its neighbours as black; this entry point drops the taps that hold nothing and FILLS the centres that hold
 * nothing from the taps that remain.  Host arrays in and out, blocking, on the current device, no scene handle, no CPU fallback.  Everything is
 * double.  (Came without a version bump: detect it by its symbol.)
 *
 * `valid`: w*h bytes, nonzero = the pixel holds a value.  The colour and the variance of a pixel with valid == 0 are NEVER READ (they may be NaN).
 * Everything else is rttnw_denoise's contract — demodulation, the taps, the weights, the parameters and their defaults — with a flag H per
 * pixel, H = (valid != 0) at first, carried through the passes:
 * Prepare (only when iterations > 0).  A pixel with H is demodulated exactly as in rttnw_denoise.  A pixel without H and with alpha == 0 takes
 *   c = albedo, variance 0 and H = 1: `albedo` is the background rttnw_render_features stores for a pixel whose every sample missed, which is what
 *   every sample of a render returns there.  Any other pixel without H keeps H = 0.
 * Pass i, stride 2^i, reads (c, v, H) and writes (c', v', H') into the other half of a ping-pong — H is ping-ponged like the colour, a pass never
 *   reads a flag it writes.
 *   A tap is dropped when it lies outside the image, has alpha == 0 or has H == 0 (so do the 3x3 taps of V, the centre's luminance variance).
 *   A centre with alpha == 0 passes through, its flag included.
 *   A centre with H: rttnw_denoise's operations, in its order, on the remaining taps; H' = 1 (a centre all of whose taps weigh 0 passes through).
 *   A centre without H: tap weight w = h_x h_y * w_n * w_z — no colour stop, it has no colour to compare.  If sum w > 0: c' = sum w c / sum w
 *     and H' = 1; with a variance input v' = sum w^2 var / (sum w)^2 over the accepted taps whose variance is finite, +inf if none is.
 *     Otherwise c' = 0 and H' = 0.
 *   Pass i reaches 2 * 2^i pixels to either side: a lattice of spacing 2^L is filled by pass L - 1 at the latest wherever the features let a
 *   neighbour through.
 * Finish.  A pixel with H is remodulated with its own albedo and alpha, as in rttnw_denoise; RGBA8 alpha 255, out_valid 1.  A pixel without H gets
 *   linear 0, 0, 0, RGBA8 0, 0, 0, 0, variance +inf and out_valid 0.  With 0 iterations a valid pixel is copied as in rttnw_denoise (no
 *   demodulation, no background fill) and an invalid one gets the outputs of a pixel without H.
 * Outputs (each optional): out_linear_rgb w*h*3, out_rgba8 w*h*4, out_variance_rgb w*h*3 (written only when variance_rgb was given), out_valid
 *   w*h bytes (0 or 1), kernel_ms: device time of the passes.
 * Contract.  With every `valid` byte nonzero the three image outputs equal rttnw_denoise's bit for bit and out_valid is all 1.  The device code, a
 *   host build of the same header (rttnw_amd/csrc/reconstruct.hpp) and a restatement in numpy give the same bits for every validity pattern.
 * Refusals, before the device is touched, each message naming `reconstruct` and the field: rttnw_denoise's, with its codes (RTTNW_ERR_INVALID for a
 *   NULL linear_rgb, albedo, normal, depth, alpha or d, width * height == 0, iterations > 8, reserved0 != 0, a negative or NaN sigma), and
 *   RTTNW_ERR_INVALID for a NULL valid. */
int rttnw_reconstruct(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const uint8_t* valid,
                      const double* albedo, const double* normal, const double* depth, const double* alpha,
                      const rttnw_denoise_params* d, double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb,
                      uint8_t* out_valid, double* kernel_ms);

/* A frame from a fraction of its pixels: an adaptive render of the LATTICE x % 2^level == 0 && y % 2^level == 0 (frame coordinates, row 0 at the
 * top; level 0 .. 6, so 1 pixel in 4^level), the features of the whole frame, and rttnw_reconstruct over the two — on the device.  A preview costs
 * bounce 0 of every pixel (the features) plus 1 / 4^level of the trace.  One GPU, tile_world == 1, blocking.  (Came without a version bump: detect
 * it by its symbol.)
 *
 * Contract.  Every output is BIT-IDENTICAL, for every `precision`, kernel form and launch split (RTTNW_CHUNK_SUM_BUDGET), to this host composition:
 *   1. rttnw_render_adaptive_region(window = the whole frame, mask = the lattice, ngpu = 0, state_in = NULL) under p's cap and a's tolerances:
 *      out_raw_linear_rgb, out_raw_stderr_rgb, out_spp and state_out are its image, standard errors, samples and state;
 *   2. F = rttnw_render_features with p->spp replaced by v->feature_spp (0 means a->pass_spp);
 *   3. rttnw_reconstruct(the raw image, variance_rgb = NULL, valid = (spp > 0), F, &v->denoise): out_linear_rgb, out_rgba8 and out_valid.
 *   The adaptive rounds use the ordinary per-pixel stopping rule under the caller's tolerances, each lattice pixel to the bits a fresh
 *   rttnw_render_adaptive gives it.  NO variance goes into the filter: at the sample counts of a preview the colour stop costs more than it protects
 *   (DESIGN.md section 10b).
 * feature_spp defaults to the pass size, not to a handful of samples: a lattice pixel's colour is DIVIDED by its albedo and the quotient is spread
 *   to the pixels around it, so an albedo estimated from other, fewer samples than the colour — near zero where the colour is not, on a noise
 *   texture — explodes there.  Features taken from the render's own first B samples are consistent with the colour they demodulate.
 * Outputs (each optional; row-major, top row first): out_linear_rgb w*h*3 the reconstructed image; out_rgba8 w*h*4 of it, alpha 0 where
 *   out_valid is 0; out_valid w*h bytes; out_spp w*h the n_q, 0 off the lattice; out_raw_linear_rgb / out_raw_stderr_rgb w*h*3 the unfiltered
 *   means and standard errors, 0 off the lattice; state_out, rttnw_adaptive_state_doubles(w, h) doubles: the ordinary adaptive state, with zero
 *   records off the lattice — rttnw_render_adaptive_region over the whole frame under the same cap and tolerances completes it to the fresh adaptive
 *   render, by that entry point's contract.  `stats`: samples = sum_q n_q, kernel_ms = device time of everything the call runs, reserved = the
 *   kernel form, the scene's sizes as usual.
 * Where it lives.  Nothing frame-sized crosses to the host before the outputs: the raw means, the features and the flags stay on the device; per
 *   round the host reads 8 bytes, the length of the round's list and the number of active pixels.
 * Refusals, before the device is touched, in this order, each message naming render_preview and the field:
 *   1. RTTNW_ERR_INVALID for a NULL p, a or v;
 *   2. what rttnw_render_adaptive refuses among its own arguments, with its codes;
 *   3. RTTNW_ERR_INVALID for v->level > 6, then v->denoise.iterations > 8, v->denoise.reserved0 != 0, a negative or NaN sigma;
 *   4. whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes).
 * Out of scope: a state_in, a node-wide form (ngpu), and windows.  A coarse-to-fine chain — level 2, then level 1, then the frame — goes through
 *   rttnw_render_adaptive_region with state_out as its state_in, and rttnw_reconstruct on what it returns. */
struct rttnw_preview {
    uint32_t level;               /* 0 .. 6: the lattice x % 2^level == 0 && y % 2^level == 0 */
    uint32_t feature_spp;         /* samples per pixel of the feature buffers; 0 = a->pass_spp */
    rttnw_denoise_params denoise; /* as rttnw_denoise: iterations 0 .. 8, sigmas (0 = the library default) */
};
typedef struct rttnw_preview rttnw_preview;
int rttnw_render_preview(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                         const rttnw_preview* v, double* out_linear_rgb, uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp,
                         double* out_raw_linear_rgb, double* out_raw_stderr_rgb, double* state_out, rttnw_stats* stats);

/* Which pixels get the next adaptive pass when not all of them can: an exact, deterministic top-m selection over a frame's pixels by noise
 * relative to tolerance — the step rttnw_render_adaptive_budget runs once per round, on its own.  Host arrays in and out, blocking, on the current
 * device, no scene handle, no CPU fallback.  (Came without a version bump: detect it by its symbol.)
 *
 * Inputs: the row-major maps every adaptive entry point returns — linear_rgb w*h*3 the means, stderr_rgb w*h*3 the standard errors (+inf with
 *   fewer than two chunks), spp w*h the sample counts.  The colour and the error of a pixel with spp == 0 are NEVER READ (they may be NaN).
 * Candidate.  Pixel q is a candidate if spp == 0, or if spp < cap and rttnw_render_adaptive's stopping rule does not hold: se_c <= abs_error +
 *   rel_error * value_c fails in some channel (the product rounded on its own, nothing fused).
 * Priority rho, a double: +inf for spp == 0; otherwise the maximum over r, g, b of e_c, where with t_c = abs_error + rel_error * value_c, e_c = 0
 *   when se_c <= t_c and se_c / t_c otherwise — and +inf where that quotient is not a finite positive number.  One product, one sum, one IEEE
 *   division and comparisons.  A candidate has rho in (1, +inf]; a non-candidate reports out_priority 0.
 * Selection.  m = min(number of candidates, max_pixels).  The selected pixels are the first m candidates in the order rho descending, then
 *   row-major index y * width + x ascending.
 * Outputs (each optional): out_mask w*h bytes, 1 for the selected pixels and 0 elsewhere; out_priority w*h doubles; out_selected = m; kernel_ms:
 *   device time of the selection.
 * How.  Every pixel gets a 96-bit key — the bit pattern of rho above 0xFFFFFFFF - index, 0 for a non-candidate —, so the selection is "the m
 *   largest keys" and has no ties; a most-significant-digit radix select finds the m-th largest with integer atomics only, so the result does not
 *   depend on scheduling.  The device code, a host build of the same header (rttnw_amd/csrc/budget_select.hpp) with a plain sort, and a restatement
 *   in numpy give the same bits.
 * Refusals, before the device is touched, each message naming `budget_select` and the field: RTTNW_ERR_INVALID for a NULL linear_rgb, stderr_rgb
 *   or spp, width * height == 0, cap == 0, a negative or NaN tolerance, both tolerances 0 (a priority relative to a tolerance of nothing ranks
 *   every noisy pixel +inf); RTTNW_ERR_UNSUPPORTED for more than 2^32 - 1 pixels (the key holds the index in 32 bits). */
int rttnw_budget_select(uint32_t width, uint32_t height, const double* linear_rgb, const double* stderr_rgb, const uint32_t* spp,
                        uint32_t cap, double rel_error, double abs_error, uint64_t max_pixels,
                        uint8_t* out_mask, double* out_priority, uint64_t* out_selected, double* kernel_ms);

/* The adaptive render under a BUDGET of samples: the other entry points of this family stop each pixel at a noise tolerance and cost what they
 * cost; this one traces at most b->samples camera paths and spends them on the worst pixels first.  One GPU, the whole frame, tile_world == 1,
 * blocking.  (Came without a version bump: detect it by its symbol.)
 *
 * B = a->pass_spp; the cap p->spp is a positive multiple of B.  The state is rttnw_render_adaptive_region's: frame-sized, a record of twelve
 * zeros means "no samples yet"; state_in == NULL stands for all zeros; state_in and state_out may be the same array.
 * Rounds.  remaining = b->samples.  Round r = 0, 1, ... runs rttnw_budget_select on the current means, standard errors and counts of every pixel,
 *   under the caller's cap and tolerances, with max_pixels = min(round_pixels, remaining / B) (integer division).  When that selects nothing the
 *   call ends.  Each selected pixel q, holding n_q samples, gets its next pass and nothing else — samples [sample_begin + n_q, sample_begin + n_q +
 *   B), with the jobs, chunk schedule, running-sum chain and noise-state update of the adaptive render's pass at level n_q / B — and remaining
 *   -= m * B.  Pixels of one round stand at different levels: the round runs one list pass per occupied level, in ascending order, over the 2x2
 *   blocks that hold a selected pixel of that level.
 * Contract.  For every `precision`, kernel form and launch split (RTTNW_CHUNK_SUM_BUDGET) the four outputs and state_out are BIT-IDENTICAL to
 *   this host composition: per round the selection restated on the host over the maps the previous step returned, then for each occupied level k,
 *   ascending, rttnw_render_adaptive_region(window = the whole frame, mask = this round's pixels at level k, ngpu = 0, cap (k+1)B, rel_error =
 *   abs_error = 0, state_in = the running state).  (That entry point refuses a state with a record above its cap: the records of the pixels
 *   that stand above level k are set aside for the call — they are not selected, it would leave them alone — and put back behind it.)  The
 *   value a pixel is ranked by is the one the adaptive render REPORTS — sum / n in the kernel's type, widened — not a division redone from the
 *   state: the f32 build's division is not correctly rounded.
 *   Two consequences.  When the budget never binds, the outputs and the state are those of rttnw_render_adaptive_resume(state_in = NULL) under the
 *   same cap, B and tolerances, bit for bit, for any round_pixels: a pixel's record is a function of its own sample count alone.  And two calls of
 *   N1 and N2 samples are NOT promised to equal one call of N1 + N2: the round the first call ended in was cut by its budget.
 * Outputs (each optional): those of rttnw_render_adaptive_region over the whole frame on the state the call ends in — a pixel without samples is
 *   zero everywhere, alpha included.  `stats`: samples = what THIS call traced, at most b->samples, and more than b->samples - B unless no
 *   candidate was left; kernel_ms = device time of everything the call runs, the state's copies included; the scene's sizes as usual; reserved =
 *   the kernel form in its low bits as usual and, in bits 16 .. 31, the rounds that traced something (saturating at 65535).
 * Where it lives.  Between rounds nothing frame-sized crosses to the host: per round the host reads one small record in one copy — the number
 *   selected and, per level, the length of the list over the selected pixels that stand at it (1 + cap / B words) — and runs only the occupied
 *   levels.
 * No work.  b->samples < B, or no candidate: RTTNW_OK, no trace kernel is launched, stats->samples == 0, the outputs are those of the incoming state.
 * Refusals, before the device is touched, in this order, each message naming render_adaptive_budget and the field:
 *   1. RTTNW_ERR_INVALID for a NULL p, a or b;
 *   2. what rttnw_render_adaptive refuses among its own arguments, with its codes;
 *   3. RTTNW_ERR_INVALID for b->reserved0 != 0, then for rel_error == abs_error == 0;
 *   4. with a state_in, the state checks of rttnw_render_adaptive_region (a record of zeros is accepted);
 *   5. whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes).
 * Out of scope: a node-wide form (ngpu), windows and masks, and ranking by the filtered error of rttnw_render_adaptive_denoised (that is
 *   rttnw_render_adaptive_budget_denoised, below). */
struct rttnw_budget {
    uint64_t samples;      /* the most camera paths THIS call may trace */
    uint32_t round_pixels; /* the most pixels one round refines; 0 = ceil(width * height / 2) */
    uint32_t reserved0;    /* must be 0 */
};
typedef struct rttnw_budget rttnw_budget;
int rttnw_render_adaptive_budget(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                                 const rttnw_budget* b, const double* state_in, double* state_out, double* out_linear_rgb,
                                 uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, rttnw_stats* stats);

/* The budgeted render ranked by the noise of the FILTERED image: rttnw_render_adaptive_budget keeps sampling smooth walls the denoiser would have
 * cleaned for free, rttnw_render_adaptive_denoised has a noise target and no budget; this one spends at most b->samples camera paths where the
 * denoised image is worst.  One GPU, the whole frame, tile_world == 1, blocking.  rttnw_budget and rttnw_guided are reused as they are.  (Came
 * without a version bump: detect it by its symbol.)
 *
 * Let B = a->pass_spp and the cap = p->spp, a positive multiple of B.  The state is rttnw_render_adaptive_region's: frame-sized, a record of twelve
 * zeros means "no samples yet"; state_in == NULL stands for all zeros; state_in and state_out may be the same array.  No "stopped" flag survives a
 * round — candidates are recomputed from the maps each round —, which is why a state_in is possible here and not in rttnw_render_adaptive_denoised.
 * Before round 0.  The features F of the frame are rttnw_render_features' with p->spp replaced by g->feature_spp (0 means B), as in
 *   rttnw_render_adaptive_denoised.  remaining = b->samples.
 * Round r = 0, 1, ...:
 *   1. Raw maps of EVERY pixel from the running state: mean = sum / n_q in the kernel's type, widened to double; se, the standard error as
 *      rttnw_render_adaptive defines it (+inf with fewer than two chunks); spp = n_q; valid = (spp > 0); variance = se * se in double, not fused.  A
 *      pixel without samples reports zeros.
 *   2. Filter.  (den, var_f, H) = rttnw_reconstruct's out_linear_rgb, out_variance_rgb and out_valid on (mean, variance, valid, F, g->denoise), bit
 *      for bit.  (With every pixel valid that is rttnw_denoise, by that entry point's contract.)
 *   3. Rank.  se_f = sqrt(var_f).  spp' = the cap for a pixel with spp > 0 whose OWN se is 0 in r, g and b — the "own stderr is 0" stop of
 *      rttnw_render_adaptive_denoised: such a pixel has nothing to gain, whatever leaks in from its neighbours —, spp' = spp otherwise.  Then
 *      rttnw_budget_select(den, se_f, spp', cap, rel_error, abs_error, max_pixels = min(round_pixels, remaining / B)) (integer division), its rules
 *      unchanged: a pixel with spp == 0 ranks +inf and its colour is never read, a quotient that is not a finite positive number ranks +inf, ties
 *      go by row-major index.
 *   4. End or trace.  When that selects nothing the call ends.  Otherwise each selected pixel q gets its next pass, at level n_q / B — one list pass
 *      per occupied level, in ascending order, exactly as in rttnw_render_adaptive_budget — and remaining -= m * B.
 *   The filter therefore runs once more than the number of rounds, and once even when there is no work.
 * Outputs, of the last filter that ran — the one whose selection was empty (each optional; row-major, top row first): out_linear_rgb w*h*3,
 *   out_rgba8 w*h*4 and out_valid w*h bytes are rttnw_reconstruct's, alpha 0 where out_valid is 0; out_stderr_rgb w*h*3 is se_f, +inf where
 *   out_valid is 0; out_raw_linear_rgb, out_raw_stderr_rgb w*h*3 and out_spp w*h are the raw maps of step 1; state_out,
 *   rttnw_adaptive_state_doubles(w, h) doubles: the ordinary adaptive state.  `stats`: samples = what THIS call traced, at most b->samples, and
 *   more than b->samples - B unless no candidate was left; kernel_ms = device time of everything the call runs — the feature pass, every filter,
 *   every selection and the state's copies included; the scene's sizes as usual; reserved = the kernel form in its low bits as usual and, in bits
 *   16 .. 31, the rounds that traced something (saturating at 65535), as in rttnw_render_adaptive_budget.
 * Contract.  For every `precision`, kernel form and launch split (RTTNW_CHUNK_SUM_BUDGET) all outputs and state_out are BIT-IDENTICAL to the host
 *   composition of steps 1 - 4 from entry points above: rttnw_render_features; rttnw_reconstruct; the selection restated on the host; and per
 *   occupied level k, ascending, rttnw_render_adaptive_region(window = the whole frame, mask = this round's pixels at level k, ngpu = 0, cap (k+1)B,
 *   rel_error = abs_error = 0, state_in = the running state), the records above that cap set aside and put back as rttnw_render_adaptive_budget's
 *   comment describes; the raw maps of step 1 are that entry point's image, standard errors and samples over the whole frame.
 *   With g->denoise.iterations == 0 the filter is the identity and sqrt(se * se) == se in IEEE double away from underflow: out_spp, state_out,
 *   the rounds, the samples and the raw maps are rttnw_render_adaptive_budget's under the same arguments, and out_linear_rgb equals the raw image.
 *   NOT promised: that two calls of N1 and N2 samples equal one call of N1 + N2 (as in rttnw_render_adaptive_budget), or equality with
 *   rttnw_render_adaptive_denoised (whose stops are sticky).
 * Where it lives.  Between rounds nothing frame-sized crosses to the host: per round the host reads the budgeted form's one small record in one
 *   copy (the number selected, then the list length per level, 1 + cap / B words).
 * No work.  b->samples < B, or no candidate: RTTNW_OK, no trace kernel is launched, stats->samples == 0, the outputs are the filter of the incoming
 *   state — with no state that is rttnw_reconstruct of nothing: only the background fill of the pixels with alpha == 0.
 * Refusals, before the device is touched, in this order, each message naming render_adaptive_budget_denoised and the field:
 *   1. RTTNW_ERR_INVALID for a NULL p, a, b or g;
 *   2. what rttnw_render_adaptive refuses among its own arguments, with its codes;
 *   3. RTTNW_ERR_INVALID for b->reserved0 != 0, then for rel_error == abs_error == 0;
 *   4. RTTNW_ERR_INVALID for g->reserved0 != 0, g->denoise.iterations > 8, g->denoise.reserved0 != 0, a negative or NaN sigma, in this order;
 *   5. with a state_in, the state checks of rttnw_render_adaptive_region (a record of zeros is accepted);
 *   6. whatever rttnw_render refuses (NULL scene / camera, a scene not committed, bad sizes).
 * Out of scope: a node-wide form (ngpu), and windows and masks. */
int rttnw_render_adaptive_budget_denoised(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                                          const rttnw_budget* b, const rttnw_guided* g, const double* state_in, double* state_out,
                                          double* out_linear_rgb, uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp,
                                          double* out_stderr_rgb, double* out_raw_linear_rgb, double* out_raw_stderr_rgb, rttnw_stats* stats);

/* Device-resident form, asynchronous on `hip_stream` (a hipStream_t; NULL = default stream).
 * Traces the tiles owned by (tile_rank, tile_world) and writes them in packed order into
 * `d_packed`: pixels_per_rank pixel records of 4 reals (mean r, g, b, 1) of the kernel's
 * arithmetic type — float for RTTNW_F32, double for RTTNW_F64.  Pad tiles are zero-filled.
 * With `stats != NULL` the call synchronises the stream to fill the device time / counters. */
int rttnw_render_tiles_device(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p,
                              void* d_packed, void* hip_stream, rttnw_stats* stats);

/* After the gather: scatter `world * pixels_per_rank` packed pixel records (rank-major, reals of
 * `precision`) into the row-major top-first framebuffer: `d_linear_rgb` = w*h*3 reals of
 * `precision` (main.rs:217), `d_rgba8` = w*h*4 bytes after main.rs:219-225 (sqrt, clamp 0.999,
 * *256, as u8, alpha 255).  Either output may be NULL.  Asynchronous on `hip_stream`. */
int rttnw_untile_device(uint32_t width, uint32_t height, uint32_t world, uint32_t precision,
                        const void* d_gathered, void* d_linear_rgb, uint8_t* d_rgba8,
                        void* hip_stream);

/* ---------------------------------------------------------------- introspection ------------ */

int rttnw_abi_version(void);
int rttnw_device_count(void);
/* Releases what the library keeps for the life of the process: the RCCL communicator sets rttnw_render_multi caches per list of
 * devices (the reference has no counterpart: rayon's pool goes with the process, main.rs:202).  Optional — the same runs at exit. */
void rttnw_shutdown(void);
const char* rttnw_last_error(void);

/* Debug/inspection: sizes of the lowered scene (valid after commit). */
int rttnw_scene_info(rttnw_scene* s, rttnw_stats* out);

/* What rttnw_scene_commit's build cost (valid after commit). */
typedef struct rttnw_build_info {
    uint32_t builder;     /* RTTNW_BVH_* */
    uint32_t n_nodes;     /* 128-byte 4-wide node records the kernels walk, all trees */
    uint32_t n_prims;     /* leaves of all trees */
    uint32_t stack_depth; /* traversal stack entries a lane needs */
    double lower_ms;      /* host wall time of the lowering, BVH builds included */
    double device_ms;     /* device time of the build kernels + sort (device builder only) */
} rttnw_build_info;
int rttnw_scene_build_info(const rttnw_scene* s, rttnw_build_info* out);

/* Debug/inspection: the BUILDERS' binary trees: copy up to max_nodes 64-byte node records (rt_types.hpp BvhNode: lo0[3]
 * hi0[3] lo1[3] hi1[3] child0 child1 pad pad; child >= 0 inner node, < 0 leaf bits) and the top-level root; returns the
 * node count.  (The kernels walk the 4-wide collapse of these trees, see rttnw_debug_scene_nodes4.) */
int rttnw_debug_scene_nodes(const rttnw_scene* s, void* out_nodes, uint32_t max_nodes, int32_t* top_root);

/* Debug/inspection: the records the kernels walk — the same trees collapsed to 4-WIDE nodes of 128 bytes (rt_types.hpp
 * Bvh4Node: lo[3][4] hi[3][4] (planes by axis, then child) child[4] pad[4]; an unused slot has child == INT32_MIN and an
 * inverted box).  Copies up to max_nodes records and the top-level root; returns the record count. */
int rttnw_debug_scene_nodes4(const rttnw_scene* s, void* out_nodes, uint32_t max_nodes, int32_t* top_root);

/* Debug/inspection: walk sample `sample` of pixel (px, row; row 0 = top) on the device with the kernels of
 * `p->precision` and dump every world.hit() of its path, 20 doubles per bounce:
 *   [0] t  [1..3] p  [4..6] normal  [7] material index  [8] u  [9] v  [10] front_face
 *   [11..13] ray origin  [14..16] ray direction  [17] ray time  [18] emitted.r  [19] attenuation.r (-1: absorbed)
 * `out` must hold max_out*20 + 4 doubles: out[max_out*20 .. +3] = the sample's radiance r,g,b (background taken
 * as black) and its final bounce count, computed by path_step(): the same walk and shade steps the trace kernels run.
 * Returns the number of bounces written (<= max_out) or a negative error.  Blocking; test use only. */
int rttnw_debug_probe_path(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p,
                           uint32_t px, uint32_t row, uint32_t sample, double* out, uint32_t max_out);

/* ---------------------------------------------------------------- entry-point table -------- */

/* Scene-building entry points as a table, so one host-side scene catalogue (the `scenes.rs`
 * mirror in rttnw_amd/host/scenes.cpp) can drive any implementation of this boundary. */
typedef struct rttnw_builder_api {
    int (*scene_create)(uint64_t, rttnw_scene**);
    void (*scene_destroy)(rttnw_scene*);
    rttnw_id (*tex_solid)(rttnw_scene*, double, double, double);
    rttnw_id (*tex_checker)(rttnw_scene*, rttnw_id, rttnw_id);
    rttnw_id (*tex_noise)(rttnw_scene*, double);
    rttnw_id (*tex_image_rgba8)(rttnw_scene*, const uint8_t*, uint32_t, uint32_t);
    rttnw_id (*mat_lambertian)(rttnw_scene*, rttnw_id);
    rttnw_id (*mat_metal)(rttnw_scene*, double, double, double, double);
    rttnw_id (*mat_dielectric)(rttnw_scene*, double);
    rttnw_id (*mat_diffuse_light)(rttnw_scene*, rttnw_id);
    rttnw_id (*mat_isotropic)(rttnw_scene*, rttnw_id);
    rttnw_id (*sphere)(rttnw_scene*, const double*, double, rttnw_id);
    rttnw_id (*moving_sphere)(rttnw_scene*, const double*, const double*, double, double, double,
                              rttnw_id);
    rttnw_id (*rectangle)(rttnw_scene*, int, double, double, double, double, double, rttnw_id);
    rttnw_id (*cube)(rttnw_scene*, const double*, const double*, rttnw_id);
    rttnw_id (*list)(rttnw_scene*);
    int (*list_push)(rttnw_scene*, rttnw_id, rttnw_id);
    rttnw_id (*bvh_tree)(rttnw_scene*, rttnw_id);
    rttnw_id (*translate)(rttnw_scene*, rttnw_id, const double*);
    rttnw_id (*rotate_y)(rttnw_scene*, rttnw_id, double);
    rttnw_id (*constant_medium)(rttnw_scene*, rttnw_id, double, rttnw_id);
    int (*scene_set_world)(rttnw_scene*, rttnw_id);
    int (*scene_commit)(rttnw_scene*);
    const char* (*last_error)(void);
} rttnw_builder_api;

const rttnw_builder_api* rttnw_builder(void);

#ifdef __cplusplus
}
#endif
#endif /* RTTNW_HIP_H */
