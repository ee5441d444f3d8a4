//! The vocabulary of the reference's `src/scenes.rs` over handles: a `SceneBuilder` whose methods are named after the
//! constructors they replace, and `render()` (src/main.rs:58-233) as one call.  Every method is one FFI call.
use crate::ffi;
use std::ffi::CStr;
use std::ptr;

#[derive(Debug)]
pub struct Error {
    pub code: i32,
    pub message: String,
}
pub type Result<T> = std::result::Result<T, Error>;

fn last_error(code: i32) -> Error {
    let message = unsafe {
        let p = ffi::rttnw_last_error();
        if p.is_null() { String::new() } else { CStr::from_ptr(p).to_string_lossy().into_owned() }
    };
    Error { code, message }
}
fn id(rc: i32) -> Result<i32> {
    if rc < 0 { Err(last_error(rc)) } else { Ok(rc) }
}
fn ok(rc: i32) -> Result<()> {
    if rc < 0 { Err(last_error(rc)) } else { Ok(()) }
}

/// `Arc<dyn Texture>` — texture.rs
#[derive(Clone, Copy, Debug)]
pub struct Tex(pub i32);
/// `Arc<dyn Material>` — material.rs
#[derive(Clone, Copy, Debug)]
pub struct Mat(pub i32);
/// `Box<dyn Hittable>` — hittable.rs
#[derive(Clone, Copy, Debug)]
pub struct Hit(pub i32);

#[derive(Clone, Copy, Debug)]
pub enum Plane {
    XY = 0,
    XZ = 1,
    YZ = 2,
}

pub struct SceneBuilder {
    raw: *mut ffi::rttnw_scene,
}

impl SceneBuilder {
    /// `scene_seed` feeds the Perlin tables the reference draws from `thread_rng()` (noise.rs:15-29,40-47).
    pub fn new(scene_seed: u64) -> Result<Self> {
        let mut raw = ptr::null_mut();
        ok(unsafe { ffi::rttnw_scene_create(scene_seed, &mut raw) })?;
        Ok(SceneBuilder { raw })
    }
    // ---- textures
    pub fn solid(&mut self, rgb: [f64; 3]) -> Result<Tex> { id(unsafe { ffi::rttnw_tex_solid(self.raw, rgb[0], rgb[1], rgb[2]) }).map(Tex) }
    pub fn checker(&mut self, odd: Tex, even: Tex) -> Result<Tex> { id(unsafe { ffi::rttnw_tex_checker(self.raw, odd.0, even.0) }).map(Tex) }
    pub fn noise(&mut self, scale: f64) -> Result<Tex> { id(unsafe { ffi::rttnw_tex_noise(self.raw, scale) }).map(Tex) }
    /// `ImageTexture::new(path)`: the host decodes (`image::open(path)?.to_rgba8()`); `None` = load failure -> cyan (texture.rs:102-105).
    pub fn image(&mut self, rgba8: Option<(&[u8], u32, u32)>) -> Result<Tex> {
        let rc = match rgba8 {
            Some((px, w, h)) => {
                assert!(px.len() as u64 == w as u64 * h as u64 * 4);
                unsafe { ffi::rttnw_tex_image_rgba8(self.raw, px.as_ptr(), w, h) }
            }
            None => unsafe { ffi::rttnw_tex_image_rgba8(self.raw, ptr::null(), 0, 0) },
        };
        id(rc).map(Tex)
    }
    // ---- materials
    pub fn lambertian(&mut self, t: Tex) -> Result<Mat> { id(unsafe { ffi::rttnw_mat_lambertian(self.raw, t.0) }).map(Mat) }
    pub fn metal(&mut self, albedo: [f64; 3], fuzz: f64) -> Result<Mat> { id(unsafe { ffi::rttnw_mat_metal(self.raw, albedo[0], albedo[1], albedo[2], fuzz) }).map(Mat) }
    pub fn dielectric(&mut self, refraction_index: f64) -> Result<Mat> { id(unsafe { ffi::rttnw_mat_dielectric(self.raw, refraction_index) }).map(Mat) }
    pub fn diffuse_light(&mut self, t: Tex) -> Result<Mat> { id(unsafe { ffi::rttnw_mat_diffuse_light(self.raw, t.0) }).map(Mat) }
    pub fn isotropic(&mut self, t: Tex) -> Result<Mat> { id(unsafe { ffi::rttnw_mat_isotropic(self.raw, t.0) }).map(Mat) }
    // ---- hittables
    pub fn sphere(&mut self, center: [f64; 3], radius: f64, m: Mat) -> Result<Hit> { id(unsafe { ffi::rttnw_sphere(self.raw, center.as_ptr(), radius, m.0) }).map(Hit) }
    pub fn moving_sphere(&mut self, center: std::ops::Range<[f64; 3]>, time: std::ops::Range<f64>, radius: f64, m: Mat) -> Result<Hit> {
        id(unsafe { ffi::rttnw_moving_sphere(self.raw, center.start.as_ptr(), center.end.as_ptr(), time.start, time.end, radius, m.0) }).map(Hit)
    }
    /// `XY|XZ|YZ::rectangle(material, a0..a1, b0..b1, k)`
    pub fn rectangle(&mut self, plane: Plane, m: Mat, a: std::ops::Range<f64>, b: std::ops::Range<f64>, k: f64) -> Result<Hit> {
        id(unsafe { ffi::rttnw_rectangle(self.raw, plane as i32, a.start, a.end, b.start, b.end, k, m.0) }).map(Hit)
    }
    pub fn cube(&mut self, min: [f64; 3], max: [f64; 3], m: Mat) -> Result<Hit> { id(unsafe { ffi::rttnw_cube(self.raw, min.as_ptr(), max.as_ptr(), m.0) }).map(Hit) }
    pub fn list(&mut self) -> Result<Hit> { id(unsafe { ffi::rttnw_list(self.raw) }).map(Hit) }
    pub fn push(&mut self, list: Hit, item: Hit) -> Result<()> { ok(unsafe { ffi::rttnw_list_push(self.raw, list.0, item.0) }) }
    /// `BvhTree::from(list)` (the list is consumed, as in the reference)
    pub fn bvh_tree(&mut self, list: Hit) -> Result<Hit> { id(unsafe { ffi::rttnw_bvh_tree(self.raw, list.0) }).map(Hit) }
    pub fn translate(&mut self, item: Hit, offset: [f64; 3]) -> Result<Hit> { id(unsafe { ffi::rttnw_translate(self.raw, item.0, offset.as_ptr()) }).map(Hit) }
    pub fn rotate_y(&mut self, item: Hit, angle_degrees: f64) -> Result<Hit> { id(unsafe { ffi::rttnw_rotate_y(self.raw, item.0, angle_degrees) }).map(Hit) }
    pub fn constant_medium(&mut self, boundary: Hit, density: f64, phase: Tex) -> Result<Hit> { id(unsafe { ffi::rttnw_constant_medium(self.raw, boundary.0, density, phase.0) }).map(Hit) }
    /// `Hittable::bounding_box(initial_time, final_time) -> Option<Bound>` (hittable.rs:50) of any hittable built so far: `Some((min, max))`, or `None`
    /// where the reference returns `None` (an empty `List`).  `YRotate`'s box is the correct rotation of the item's corners (not quirk Q2's).
    pub fn bounding_box(&self, item: Hit, time: std::ops::Range<f64>) -> Result<Option<([f64; 3], [f64; 3])>> {
        let mut b = [0f64; 6];
        let rc = unsafe { ffi::rttnw_hittable_bounds(self.raw, item.0, time.start, time.end, b.as_mut_ptr()) };
        if rc < 0 { return ok(rc).map(|_| None); }
        Ok(if rc == 1 { Some(([b[0], b[1], b[2]], [b[3], b[4], b[5]])) } else { None })
    }
    /// Force where the BVHs are built; before `commit`.  Without this call the library decides per tree (`RTTNW_BVH_AUTO`: host below
    /// 100 000 leaves, the device's binned-SAH build above).
    pub fn device_bvh(&mut self, on: bool) -> Result<()> {
        ok(unsafe { ffi::rttnw_scene_set_bvh_builder(self.raw, if on { ffi::RTTNW_BVH_DEVICE_SAH } else { ffi::RTTNW_BVH_HOST_SAH }) })
    }
    /// `Scene { world, .. }` is complete: lower, build, upload.
    pub fn commit(mut self, world: Hit) -> Result<Scene> {
        ok(unsafe { ffi::rttnw_scene_set_world(self.raw, world.0) })?;
        ok(unsafe { ffi::rttnw_scene_commit(self.raw) })?;
        let raw = std::mem::replace(&mut self.raw, ptr::null_mut());
        Ok(Scene { raw })
    }
}
impl Drop for SceneBuilder {
    fn drop(&mut self) {
        if !self.raw.is_null() { unsafe { ffi::rttnw_scene_destroy(self.raw) } }
    }
}

/// A committed, immutable scene resident on the device(s).
pub struct Scene {
    raw: *mut ffi::rttnw_scene,
}
unsafe impl Send for Scene {}

/// The constants of `render()` (main.rs:184-197,216,33) with the reference's values.
pub fn reference_params(width: u32, height: u32, samples: u32, background: [f64; 3]) -> ffi::rttnw_params {
    ffi::rttnw_params {
        width, height, spp: samples, max_depth: 50, t_min: 0.001, background, seed: 1,
        precision: ffi::RTTNW_F64, quirks: ffi::RTTNW_QUIRKS_REFERENCE, spp_chunk: 0, tile_rank: 0, tile_world: 1,
        collect_counters: 0, sample_begin: 0, reserved0: 0,
    }
}
pub fn reference_camera(lookfrom: [f64; 3], lookat: [f64; 3], vertical_fov: f64, aspect_ratio: f64, aperture: f64) -> ffi::rttnw_camera_desc {
    ffi::rttnw_camera_desc {
        lookfrom, lookat, view_up: [0.0, 1.0, 0.0], vertical_fov, aspect_ratio, aperture,
        focus_distance: 10.0, open_time: 0.0, close_time: 1.0, // main.rs:185-196
    }
}

impl Scene {
    /// `render()` on one GPU: RGBA8, row-major, top row first (main.rs:202-229).
    pub fn render(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params) -> Result<(Vec<u8>, ffi::rttnw_stats)> {
        let mut rgba = vec![0u8; p.width as usize * p.height as usize * 4];
        let mut stats = ffi::rttnw_stats::default();
        ok(unsafe { ffi::rttnw_render(self.raw, cam, p, ptr::null_mut(), rgba.as_mut_ptr(), &mut stats) })?;
        Ok((rgba, stats))
    }
    /// Adaptive sampling on one GPU: passes of `a.pass_spp` samples until every pixel meets `a`'s noise bound or has `p.spp` samples.
    /// Returns (RGBA8, samples per pixel, standard error of each pixel's mean per channel, stats), row-major, top row first.
    pub fn render_adaptive(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive) -> Result<(Vec<u8>, Vec<u32>, Vec<f64>, ffi::rttnw_stats)> {
        let n = p.width as usize * p.height as usize;
        let mut rgba = vec![0u8; n * 4];
        let mut spp = vec![0u32; n];
        let mut stderr = vec![0f64; n * 3];
        let mut stats = ffi::rttnw_stats::default();
        ok(unsafe { ffi::rttnw_render_adaptive(self.raw, cam, p, a, ptr::null_mut(), rgba.as_mut_ptr(), spp.as_mut_ptr(), stderr.as_mut_ptr(), &mut stats) })?;
        Ok((rgba, spp, stderr, stats))
    }
    /// The same adaptive render from the GPUs `devices` of this node (`rttnw_render_adaptive_multi`): bit-identical outputs, one stats record
    /// per rank (a device may repeat: logical ranks).
    pub fn render_adaptive_multi(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive, devices: &[i32]) -> Result<(Vec<u8>, Vec<u32>, Vec<f64>, Vec<ffi::rttnw_stats>)> {
        let n = p.width as usize * p.height as usize;
        let mut rgba = vec![0u8; n * 4];
        let mut spp = vec![0u32; n];
        let mut stderr = vec![0f64; n * 3];
        let mut stats = vec![ffi::rttnw_stats::default(); devices.len()];
        ok(unsafe { ffi::rttnw_render_adaptive_multi(self.raw, cam, p, a, devices.len() as u32, devices.as_ptr(), ptr::null_mut(), rgba.as_mut_ptr(), spp.as_mut_ptr(), stderr.as_mut_ptr(), stats.as_mut_ptr()) })?;
        Ok((rgba, spp, stderr, stats))
    }
    /// The adaptive render begun from `state` (what an earlier call returned; `None`: a fresh render) and continued under `a` and the cap `p.spp`
    /// (`rttnw_render_adaptive_resume`): with a cap and tolerances no looser than the state's, bit for bit the render that was never interrupted.
    /// `devices` empty: the scene's device, one stats record; otherwise the ranks of `render_adaptive_multi`.  The state does not identify the
    /// scene: resume on the scene it was made on.  Returns (RGBA8, samples per pixel, standard errors, stats, the state to resume from).
    pub fn render_adaptive_resume(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive, devices: &[i32], state: Option<&[f64]>) -> Result<(Vec<u8>, Vec<u32>, Vec<f64>, Vec<ffi::rttnw_stats>, Vec<f64>)> {
        let n = p.width as usize * p.height as usize;
        let doubles = unsafe { ffi::rttnw_adaptive_state_doubles(p.width, p.height) } as usize;
        if state.map_or(false, |s| s.len() != doubles) {
            return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "render_adaptive_resume: the state does not have the frame's size".into() });
        }
        let mut rgba = vec![0u8; n * 4];
        let mut spp = vec![0u32; n];
        let mut stderr = vec![0f64; n * 3];
        let mut stats = vec![ffi::rttnw_stats::default(); devices.len().max(1)];
        let mut out = vec![0f64; doubles];
        let ids = if devices.is_empty() { ptr::null() } else { devices.as_ptr() };
        ok(unsafe { ffi::rttnw_render_adaptive_resume(self.raw, cam, p, a, devices.len() as u32, ids, state.map_or(ptr::null(), |s| s.as_ptr()), out.as_mut_ptr(), ptr::null_mut(), rgba.as_mut_ptr(), spp.as_mut_ptr(), stderr.as_mut_ptr(), stats.as_mut_ptr()) })?;
        Ok((rgba, spp, stderr, stats, out))
    }
    /// The adaptive render over pixels `[x0, x1) x [y0, y1)` of the frame, or those of them whose byte of `mask` (window-sized, row-major, top row
    /// first) is nonzero (`rttnw_render_adaptive_region`), begun from `state` — frame-sized, as `render_adaptive_resume` returns it, a pixel never
    /// sampled being a record of zeros; `None`: all zeros.  Only selected pixels are traced, each to the bits of a fresh whole-frame adaptive
    /// render under `a` and the cap `p.spp`; the others keep their records.  `devices` as in `render_adaptive_resume`.
    /// Returns (RGBA8, samples per pixel and standard errors of the window — a pixel without samples is zero, alpha included —, stats, the state).
    pub fn render_adaptive_region(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive, x0: u32, y0: u32, x1: u32, y1: u32, mask: Option<&[u8]>, devices: &[i32], state: Option<&[f64]>) -> Result<(Vec<u8>, Vec<u32>, Vec<f64>, Vec<ffi::rttnw_stats>, Vec<f64>)> {
        let n = (x1.saturating_sub(x0) as usize) * (y1.saturating_sub(y0) as usize);
        if mask.map_or(false, |m| m.len() != n) {
            return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "render_adaptive_region: the mask does not have the window's size".into() });
        }
        let doubles = unsafe { ffi::rttnw_adaptive_state_doubles(p.width, p.height) } as usize;
        if state.map_or(false, |s| s.len() != doubles) {
            return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "render_adaptive_region: the state does not have the frame's size".into() });
        }
        let mut rgba = vec![0u8; n * 4];
        let mut spp = vec![0u32; n];
        let mut stderr = vec![0f64; n * 3];
        let mut stats = vec![ffi::rttnw_stats::default(); devices.len().max(1)];
        let mut out = vec![0f64; doubles];
        let ids = if devices.is_empty() { ptr::null() } else { devices.as_ptr() };
        ok(unsafe { ffi::rttnw_render_adaptive_region(self.raw, cam, p, a, x0, y0, x1, y1, mask.map_or(ptr::null(), |m| m.as_ptr()), devices.len() as u32, ids, state.map_or(ptr::null(), |s| s.as_ptr()), out.as_mut_ptr(), ptr::null_mut(), rgba.as_mut_ptr(), spp.as_mut_ptr(), stderr.as_mut_ptr(), stats.as_mut_ptr()) })?;
        Ok((rgba, spp, stderr, stats, out))
    }
    /// Adaptive sampling stopped on the noise of the FILTERED image (`rttnw_render_adaptive_denoised`): the adaptive rounds and `denoise`'s passes
    /// alternate on the device, on one GPU.  Returns (the denoised image as RGBA8, samples per pixel, sqrt of the filtered variance, stats, the
    /// state, which `render_adaptive_resume` accepts).
    pub fn render_adaptive_denoised(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive, g: &ffi::rttnw_guided) -> Result<(Vec<u8>, Vec<u32>, Vec<f64>, ffi::rttnw_stats, Vec<f64>)> {
        let n = p.width as usize * p.height as usize;
        let doubles = unsafe { ffi::rttnw_adaptive_state_doubles(p.width, p.height) } as usize;
        let mut rgba = vec![0u8; n * 4];
        let mut spp = vec![0u32; n];
        let mut stderr = vec![0f64; n * 3];
        let mut stats = ffi::rttnw_stats::default();
        let mut out = vec![0f64; doubles];
        ok(unsafe { ffi::rttnw_render_adaptive_denoised(self.raw, cam, p, a, g, ptr::null_mut(), rgba.as_mut_ptr(), spp.as_mut_ptr(), stderr.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), out.as_mut_ptr(), &mut stats) })?;
        Ok((rgba, spp, stderr, stats, out))
    }
    /// A frame from 1 pixel in 4^level (`rttnw_render_preview`): the adaptive render of the lattice `x % 2^level == 0 && y % 2^level == 0`, the
    /// features of the whole frame and `reconstruct` over the two, on the device, on one GPU.  Returns (the reconstructed image as RGBA8, the
    /// byte per pixel that says whether it holds a value, samples per pixel — 0 off the lattice —, stats, the state with zero records off the
    /// lattice, which `render_adaptive_region` over the whole frame completes).
    pub fn render_preview(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive, v: &ffi::rttnw_preview) -> Result<(Vec<u8>, Vec<u8>, Vec<u32>, ffi::rttnw_stats, Vec<f64>)> {
        let n = p.width as usize * p.height as usize;
        let doubles = unsafe { ffi::rttnw_adaptive_state_doubles(p.width, p.height) } as usize;
        let mut rgba = vec![0u8; n * 4];
        let mut valid = vec![0u8; n];
        let mut spp = vec![0u32; n];
        let mut stats = ffi::rttnw_stats::default();
        let mut out = vec![0f64; doubles];
        ok(unsafe { ffi::rttnw_render_preview(self.raw, cam, p, a, v, ptr::null_mut(), rgba.as_mut_ptr(), valid.as_mut_ptr(), spp.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), out.as_mut_ptr(), &mut stats) })?;
        Ok((rgba, valid, spp, stats, out))
    }
    /// The adaptive render under a budget of samples (`rttnw_render_adaptive_budget`): at most `b.samples` camera paths, spent in rounds on the
    /// pixels `budget_select` ranks worst under `a` and the cap `p.spp`, begun from `state` (frame-sized, a pixel never sampled being a record
    /// of zeros; `None`: all zeros), on one GPU.  Returns (RGBA8, samples per pixel and standard errors — a pixel without samples is zero, alpha
    /// included —, stats, the state, the rounds run).
    pub fn render_adaptive_budget(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive, b: &ffi::rttnw_budget, state: Option<&[f64]>) -> Result<(Vec<u8>, Vec<u32>, Vec<f64>, ffi::rttnw_stats, Vec<f64>, u32)> {
        let n = p.width as usize * p.height as usize;
        let doubles = unsafe { ffi::rttnw_adaptive_state_doubles(p.width, p.height) } as usize;
        if state.map_or(false, |s| s.len() != doubles) {
            return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "render_adaptive_budget: the state does not have the frame's size".into() });
        }
        let mut rgba = vec![0u8; n * 4];
        let mut spp = vec![0u32; n];
        let mut stderr = vec![0f64; n * 3];
        let mut stats = ffi::rttnw_stats::default();
        let mut out = vec![0f64; doubles];
        ok(unsafe { ffi::rttnw_render_adaptive_budget(self.raw, cam, p, a, b, state.map_or(ptr::null(), |s| s.as_ptr()), out.as_mut_ptr(), ptr::null_mut(), rgba.as_mut_ptr(), spp.as_mut_ptr(), stderr.as_mut_ptr(), &mut stats) })?;
        let rounds = stats.reserved >> 16;
        Ok((rgba, spp, stderr, stats, out, rounds))
    }
    /// The budgeted render ranked by the noise of the FILTERED image (`rttnw_render_adaptive_budget_denoised`): `render_adaptive_budget`'s rounds,
    /// each of which runs `reconstruct`'s passes on the device and ranks pixels on the filtered image and sqrt of the filtered variance, begun
    /// from `state` (`None`: all zeros), on one GPU.  Returns (the filtered image as RGBA8, the byte per pixel that says whether it holds a value,
    /// samples per pixel, sqrt of the filtered variance, stats, the state, the rounds run).
    pub fn render_adaptive_budget_denoised(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, a: &ffi::rttnw_adaptive, b: &ffi::rttnw_budget, g: &ffi::rttnw_guided, state: Option<&[f64]>) -> Result<(Vec<u8>, Vec<u8>, Vec<u32>, Vec<f64>, ffi::rttnw_stats, Vec<f64>, u32)> {
        let n = p.width as usize * p.height as usize;
        let doubles = unsafe { ffi::rttnw_adaptive_state_doubles(p.width, p.height) } as usize;
        if state.map_or(false, |s| s.len() != doubles) {
            return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "render_adaptive_budget_denoised: the state does not have the frame's size".into() });
        }
        let mut rgba = vec![0u8; n * 4];
        let mut valid = vec![0u8; n];
        let mut spp = vec![0u32; n];
        let mut stderr = vec![0f64; n * 3];
        let mut stats = ffi::rttnw_stats::default();
        let mut out = vec![0f64; doubles];
        ok(unsafe { ffi::rttnw_render_adaptive_budget_denoised(self.raw, cam, p, a, b, g, state.map_or(ptr::null(), |s| s.as_ptr()), out.as_mut_ptr(), ptr::null_mut(), rgba.as_mut_ptr(), valid.as_mut_ptr(), spp.as_mut_ptr(), stderr.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), &mut stats) })?;
        let rounds = stats.reserved >> 16;
        Ok((rgba, valid, spp, stderr, stats, out, rounds))
    }
    /// First-hit feature buffers of the frame `render` renders (`rttnw_render_features`), row-major, top row first.
    pub fn render_features(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params) -> Result<Features> {
        let n = p.width as usize * p.height as usize;
        let mut f = Features { width: p.width, height: p.height, albedo: vec![0f64; n * 3], normal: vec![0f64; n * 3], depth: vec![0f64; n], alpha: vec![0f64; n] };
        ok(unsafe { ffi::rttnw_render_features(self.raw, cam, p, f.albedo.as_mut_ptr(), f.normal.as_mut_ptr(), f.depth.as_mut_ptr(), f.alpha.as_mut_ptr(), ptr::null_mut()) })?;
        Ok(f)
    }
    /// Pixels `[x0, x1) x [y0, y1)` of the frame `render` renders (`rttnw_render_region`): all of them, or those whose byte of `mask`
    /// (window-sized, row-major, top row first) is nonzero — each bit-identical to the full render's; an unselected pixel is 0, 0, 0, 0.
    /// Returns (RGBA8 of the window, row-major, top row first; stats).
    pub fn render_region(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, x0: u32, y0: u32, x1: u32, y1: u32, mask: Option<&[u8]>) -> Result<(Vec<u8>, ffi::rttnw_stats)> {
        let n = (x1.saturating_sub(x0) as usize) * (y1.saturating_sub(y0) as usize);
        if mask.map_or(false, |m| m.len() != n) {
            return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "render_region: the mask does not have the window's size".into() });
        }
        let mut rgba = vec![0u8; n * 4];
        let mut stats = ffi::rttnw_stats::default();
        ok(unsafe { ffi::rttnw_render_region(self.raw, cam, p, x0, y0, x1, y1, mask.map_or(ptr::null(), |m| m.as_ptr()), ptr::null_mut(), rgba.as_mut_ptr(), &mut stats) })?;
        Ok((rgba, stats))
    }
    /// The same image from the GPUs `devices` of this node (tile partition + RCCL gather inside the library).
    pub fn render_multi(&self, cam: &ffi::rttnw_camera_desc, p: &ffi::rttnw_params, devices: &[i32]) -> Result<(Vec<u8>, Vec<ffi::rttnw_stats>)> {
        let mut rgba = vec![0u8; p.width as usize * p.height as usize * 4];
        let mut stats = vec![ffi::rttnw_stats::default(); devices.len()];
        ok(unsafe { ffi::rttnw_render_multi(self.raw, cam, p, devices.len() as u32, devices.as_ptr(), ptr::null_mut(), rgba.as_mut_ptr(), stats.as_mut_ptr()) })?;
        Ok((rgba, stats))
    }
    pub fn build_info(&self) -> Result<ffi::rttnw_build_info> {
        let mut bi = ffi::rttnw_build_info::default();
        ok(unsafe { ffi::rttnw_scene_build_info(self.raw, &mut bi) })?;
        Ok(bi)
    }
}
/// What `Scene::render_features` returns: albedo and normal w*h*3, depth and alpha w*h.
pub struct Features {
    pub width: u32,
    pub height: u32,
    pub albedo: Vec<f64>,
    pub normal: Vec<f64>,
    pub depth: Vec<f64>,
    pub alpha: Vec<f64>,
}

/// `rttnw_denoise`: the feature-guided a-trous filter over a linear image (w*h*3); `variance` is the variance of the pixel means (the
/// square of `render_adaptive`'s standard errors).  Returns (linear w*h*3, RGBA8 w*h*4).
pub fn denoise(linear: &[f64], variance: Option<&[f64]>, f: &Features, d: &ffi::rttnw_denoise_params) -> Result<(Vec<f64>, Vec<u8>)> {
    let n = f.width as usize * f.height as usize;
    if linear.len() != n * 3 || variance.map_or(false, |v| v.len() != n * 3) || f.albedo.len() != n * 3 || f.normal.len() != n * 3 || f.depth.len() != n || f.alpha.len() != n {
        return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "denoise: array sizes do not match the image".into() });
    }
    let mut out = vec![0f64; n * 3];
    let mut rgba = vec![0u8; n * 4];
    ok(unsafe {
        ffi::rttnw_denoise(f.width, f.height, linear.as_ptr(), variance.map_or(ptr::null(), |v| v.as_ptr()), f.albedo.as_ptr(), f.normal.as_ptr(), f.depth.as_ptr(),
                           f.alpha.as_ptr(), d, out.as_mut_ptr(), rgba.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())
    })?;
    Ok((out, rgba))
}

/// What `denoise_nlm` returns: the filtered image (linear w*h*3 and RGBA8 w*h*4), the two cross-filtered halves and (a' - b')^2 / 4, w*h*3 each.
pub struct NlmOutput {
    pub linear: Vec<f64>,
    pub rgba8: Vec<u8>,
    pub half_a: Vec<f64>,
    pub half_b: Vec<f64>,
    pub error: Vec<f64>,
}

/// `rttnw_denoise_nlm`: non-local means over two half-buffers (w*h*3 each: the means of two disjoint, equally large sample sets); the weights that
/// average one half are patch distances measured in the other.  `variances`: the variance of each half's pixel means, or None for the pair variance.
pub fn denoise_nlm(width: u32, height: u32, half_a: &[f64], half_b: &[f64], variances: Option<(&[f64], &[f64])>, d: &ffi::rttnw_nlm_params) -> Result<NlmOutput> {
    let n = width as usize * height as usize;
    if half_a.len() != n * 3 || half_b.len() != n * 3 || variances.map_or(false, |(va, vb)| va.len() != n * 3 || vb.len() != n * 3) {
        return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "denoise_nlm: array sizes do not match the image".into() });
    }
    let mut out = NlmOutput { linear: vec![0f64; n * 3], rgba8: vec![0u8; n * 4], half_a: vec![0f64; n * 3], half_b: vec![0f64; n * 3], error: vec![0f64; n * 3] };
    ok(unsafe {
        ffi::rttnw_denoise_nlm(width, height, half_a.as_ptr(), half_b.as_ptr(), variances.map_or(ptr::null(), |v| v.0.as_ptr()), variances.map_or(ptr::null(), |v| v.1.as_ptr()),
                               d, out.linear.as_mut_ptr(), out.rgba8.as_mut_ptr(), out.half_a.as_mut_ptr(), out.half_b.as_mut_ptr(), out.error.as_mut_ptr(), ptr::null_mut())
    })?;
    Ok(out)
}

/// What `denoise_select` returns: the blended image (linear w*h*3 and RGBA8 w*h*4), the weight of non-local means per pixel (w*h, 0 .. 1), the
/// mean of each filter's two filtered halves and the error estimate, w*h*3 each.
pub struct SelectOutput {
    pub linear: Vec<f64>,
    pub rgba8: Vec<u8>,
    pub blend: Vec<f64>,
    pub feature: Vec<f64>,
    pub nlm: Vec<f64>,
    pub error: Vec<f64>,
}

/// `rttnw_denoise_select`: per pixel, the better of `denoise` (guided by `f`) and `denoise_nlm` over two half-buffers (w*h*3 each): a filtered
/// half is scored against the other, raw half.  `variances`: the variance of each half's pixel means, given to both filters, or None.
pub fn denoise_select(half_a: &[f64], half_b: &[f64], variances: Option<(&[f64], &[f64])>, f: &Features, dn: &ffi::rttnw_denoise_params, nl: &ffi::rttnw_nlm_params,
                      sel: &ffi::rttnw_select_params) -> Result<SelectOutput> {
    let n = f.width as usize * f.height as usize;
    if half_a.len() != n * 3 || half_b.len() != n * 3 || variances.map_or(false, |(va, vb)| va.len() != n * 3 || vb.len() != n * 3) || f.albedo.len() != n * 3
        || f.normal.len() != n * 3 || f.depth.len() != n || f.alpha.len() != n {
        return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "denoise_select: array sizes do not match the image".into() });
    }
    let mut out = SelectOutput { linear: vec![0f64; n * 3], rgba8: vec![0u8; n * 4], blend: vec![0f64; n], feature: vec![0f64; n * 3], nlm: vec![0f64; n * 3],
                                 error: vec![0f64; n * 3] };
    ok(unsafe {
        ffi::rttnw_denoise_select(f.width, f.height, half_a.as_ptr(), half_b.as_ptr(), variances.map_or(ptr::null(), |v| v.0.as_ptr()),
                                  variances.map_or(ptr::null(), |v| v.1.as_ptr()), f.albedo.as_ptr(), f.normal.as_ptr(), f.depth.as_ptr(), f.alpha.as_ptr(), dn, nl, sel,
                                  out.linear.as_mut_ptr(), out.rgba8.as_mut_ptr(), out.blend.as_mut_ptr(), out.feature.as_mut_ptr(), out.nlm.as_mut_ptr(),
                                  out.error.as_mut_ptr(), ptr::null_mut())
    })?;
    Ok(out)
}

/// What `temporal_accumulate` returns, and what the next call takes as its history beside that frame's features and camera: the accumulated image
/// (linear w*h*3 and RGBA8 w*h*4), its variance (w*h*3, with variances only), the frames each pixel's history counts (w*h) and where each pixel was
/// in the previous frame (w*h*2, NaN without a history: a motion-vector map).
pub struct TemporalOutput {
    pub linear: Vec<f64>,
    pub rgba8: Vec<u8>,
    pub variance: Option<Vec<f64>>,
    pub length: Vec<f64>,
    pub prev_xy: Vec<f64>,
}

/// The previous frame as `temporal_accumulate` reads it: the previous call's output, that frame's features and its camera.
pub struct TemporalHistory<'a> {
    pub output: &'a TemporalOutput,
    pub features: &'a Features,
    pub cam: &'a ffi::rttnw_camera_desc,
}

/// `rttnw_temporal_accumulate`: this frame (`linear` w*h*3, `variance` of its pixel means or None, its features `f`, its camera) blended with the
/// history, which is fetched from where each pixel's surface point was in the previous frame; None starts a sequence.  Beside a history the
/// variances come both or neither.
pub fn temporal_accumulate(linear: &[f64], variance: Option<&[f64]>, f: &Features, cam: &ffi::rttnw_camera_desc, history: Option<&TemporalHistory>,
                           t: &ffi::rttnw_temporal_params) -> Result<TemporalOutput> {
    let n = f.width as usize * f.height as usize;
    let fits = |g: &Features| g.width == f.width && g.height == f.height && g.normal.len() == n * 3 && g.depth.len() == n && g.alpha.len() == n;
    if linear.len() != n * 3 || variance.map_or(false, |v| v.len() != n * 3) || !fits(f)
        || history.map_or(false, |h| !fits(h.features) || h.output.linear.len() != n * 3 || h.output.length.len() != n
                                     || h.output.variance.as_ref().map_or(false, |v| v.len() != n * 3)) {
        return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "temporal_accumulate: array sizes do not match the image".into() });
    }
    let mut out = TemporalOutput { linear: vec![0f64; n * 3], rgba8: vec![0u8; n * 4], variance: variance.map(|_| vec![0f64; n * 3]), length: vec![0f64; n],
                                   prev_xy: vec![0f64; n * 2] };
    let null = ptr::null::<f64>();
    ok(unsafe {
        ffi::rttnw_temporal_accumulate(f.width, f.height, cam, history.map_or(ptr::null(), |h| h.cam as *const _), linear.as_ptr(),
                                       variance.map_or(null, |v| v.as_ptr()), f.normal.as_ptr(), f.depth.as_ptr(), f.alpha.as_ptr(),
                                       history.map_or(null, |h| h.output.linear.as_ptr()),
                                       history.and_then(|h| h.output.variance.as_ref()).map_or(null, |v| v.as_ptr()),
                                       history.map_or(null, |h| h.output.length.as_ptr()), history.map_or(null, |h| h.features.normal.as_ptr()),
                                       history.map_or(null, |h| h.features.depth.as_ptr()), history.map_or(null, |h| h.features.alpha.as_ptr()), t,
                                       out.linear.as_mut_ptr(), out.rgba8.as_mut_ptr(), out.variance.as_mut().map_or(ptr::null_mut(), |v| v.as_mut_ptr()),
                                       out.length.as_mut_ptr(), out.prev_xy.as_mut_ptr(), ptr::null_mut())
    })?;
    Ok(out)
}

/// What `temporal_variance` returns, and what the next call takes as its history beside that frame's features and camera: the accumulated image
/// (linear w*h*3 and RGBA8 w*h*4), the accumulated second moment of the colour (w*h*3), the frames each pixel's history counts (w*h), where each
/// pixel was in the previous frame (w*h*2, NaN without a history) and the variance of the pixel means (w*h*3), which `denoise` takes as its variance.
pub struct VarianceOutput {
    pub linear: Vec<f64>,
    pub rgba8: Vec<u8>,
    pub moment2: Vec<f64>,
    pub length: Vec<f64>,
    pub prev_xy: Vec<f64>,
    pub variance: Vec<f64>,
}

/// The previous frame as `temporal_variance` reads it: the previous call's output, that frame's features and its camera.
pub struct VarianceHistory<'a> {
    pub output: &'a VarianceOutput,
    pub features: &'a Features,
    pub cam: &'a ffi::rttnw_camera_desc,
}

/// `rttnw_temporal_variance`: `temporal_accumulate` of this frame without variances, the colour's second moment carried along the same history, and
/// the variance of every pixel's accumulated mean: from the two moments where the history is long enough, from a window guided by normal and depth
/// elsewhere.  None starts a sequence.
pub fn temporal_variance(linear: &[f64], f: &Features, cam: &ffi::rttnw_camera_desc, history: Option<&VarianceHistory>, t: &ffi::rttnw_temporal_params,
                         v: &ffi::rttnw_variance_params) -> Result<VarianceOutput> {
    let n = f.width as usize * f.height as usize;
    let fits = |g: &Features| g.width == f.width && g.height == f.height && g.normal.len() == n * 3 && g.depth.len() == n && g.alpha.len() == n;
    if linear.len() != n * 3 || !fits(f)
        || history.map_or(false, |h| !fits(h.features) || h.output.linear.len() != n * 3 || h.output.moment2.len() != n * 3 || h.output.length.len() != n) {
        return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "temporal_variance: array sizes do not match the image".into() });
    }
    let mut out = VarianceOutput { linear: vec![0f64; n * 3], rgba8: vec![0u8; n * 4], moment2: vec![0f64; n * 3], length: vec![0f64; n],
                                   prev_xy: vec![0f64; n * 2], variance: vec![0f64; n * 3] };
    let null = ptr::null::<f64>();
    ok(unsafe {
        ffi::rttnw_temporal_variance(f.width, f.height, cam, history.map_or(ptr::null(), |h| h.cam as *const _), linear.as_ptr(), f.normal.as_ptr(),
                                     f.depth.as_ptr(), f.alpha.as_ptr(), history.map_or(null, |h| h.output.linear.as_ptr()),
                                     history.map_or(null, |h| h.output.moment2.as_ptr()), history.map_or(null, |h| h.output.length.as_ptr()),
                                     history.map_or(null, |h| h.features.normal.as_ptr()), history.map_or(null, |h| h.features.depth.as_ptr()),
                                     history.map_or(null, |h| h.features.alpha.as_ptr()), t, v, out.linear.as_mut_ptr(), out.rgba8.as_mut_ptr(),
                                     out.moment2.as_mut_ptr(), out.length.as_mut_ptr(), out.prev_xy.as_mut_ptr(), out.variance.as_mut_ptr(), ptr::null_mut())
    })?;
    Ok(out)
}

/// `rttnw_reconstruct`: `denoise` over an image of which only the pixels with a nonzero byte in `valid` (w*h) hold a value; `linear` and
/// `variance` are never read elsewhere.  Returns (linear w*h*3, RGBA8 w*h*4 with alpha 0 where nothing could be filled, the valid bytes).
pub fn reconstruct(linear: &[f64], variance: Option<&[f64]>, valid: &[u8], f: &Features, d: &ffi::rttnw_denoise_params) -> Result<(Vec<f64>, Vec<u8>, Vec<u8>)> {
    let n = f.width as usize * f.height as usize;
    if linear.len() != n * 3 || variance.map_or(false, |v| v.len() != n * 3) || valid.len() != n || f.albedo.len() != n * 3 || f.normal.len() != n * 3 || f.depth.len() != n
        || f.alpha.len() != n {
        return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "reconstruct: array sizes do not match the image".into() });
    }
    let mut out = vec![0f64; n * 3];
    let mut rgba = vec![0u8; n * 4];
    let mut out_valid = vec![0u8; n];
    ok(unsafe {
        ffi::rttnw_reconstruct(f.width, f.height, linear.as_ptr(), variance.map_or(ptr::null(), |v| v.as_ptr()), valid.as_ptr(), f.albedo.as_ptr(), f.normal.as_ptr(),
                               f.depth.as_ptr(), f.alpha.as_ptr(), d, out.as_mut_ptr(), rgba.as_mut_ptr(), ptr::null_mut(), out_valid.as_mut_ptr(), ptr::null_mut())
    })?;
    Ok((out, rgba, out_valid))
}

/// `rttnw_budget_select`: which pixels get the next adaptive pass when only `max_pixels` of them can — the candidates under `cap` and the
/// tolerances, ranked by standard error over tolerance, then by row-major index.  `linear` and `stderr` (w*h*3) are never read where `spp` (w*h)
/// is 0.  Returns (the mask w*h, the priorities w*h — 0 for a non-candidate, +inf for a pixel without samples —, the number selected).
pub fn budget_select(width: u32, height: u32, linear: &[f64], stderr: &[f64], spp: &[u32], cap: u32, rel_error: f64, abs_error: f64, max_pixels: u64) -> Result<(Vec<u8>, Vec<f64>, u64)> {
    let n = width as usize * height as usize;
    if linear.len() != n * 3 || stderr.len() != n * 3 || spp.len() != n {
        return Err(Error { code: ffi::RTTNW_ERR_INVALID, message: "budget_select: array sizes do not match the image".into() });
    }
    let mut mask = vec![0u8; n];
    let mut priority = vec![0f64; n];
    let mut selected = 0u64;
    ok(unsafe { ffi::rttnw_budget_select(width, height, linear.as_ptr(), stderr.as_ptr(), spp.as_ptr(), cap, rel_error, abs_error, max_pixels, mask.as_mut_ptr(), priority.as_mut_ptr(), &mut selected, ptr::null_mut()) })?;
    Ok((mask, priority, selected))
}

impl Drop for Scene {
    fn drop(&mut self) {
        if !self.raw.is_null() { unsafe { ffi::rttnw_scene_destroy(self.raw) } }
    }
}
