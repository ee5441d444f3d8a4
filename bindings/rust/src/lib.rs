//! `rttnw-hip`: what `src/math/` of luliic2/rttnw becomes when the tracing core runs on an MI355X.
//!
//! * [`ffi`] — `include/rttnw_hip.h`, declaration for declaration (held against the header by a test).
//! * [`scene`] — handles and a builder with the vocabulary of the reference's `scenes.rs`
//!   (`Sphere {..}` -> `b.sphere(..)`, `.rotate_y(a).translate(v)` -> `b.translate(b.rotate_y(x, a), v)`), and
//!   `render()` as one call.
pub mod ffi;
pub mod scene;

/// The filters that need no scene handle, at the crate's root: the feature-guided one, non-local means over two half-buffers, the
/// per-pixel choice between the two, the accumulation of a frame with the reprojected previous one, and that accumulation with the variance
/// of every pixel's mean estimated from the history.
pub use scene::{denoise, denoise_nlm, denoise_select, temporal_accumulate, temporal_variance, NlmOutput, SelectOutput, TemporalHistory, TemporalOutput,
                VarianceHistory, VarianceOutput};
