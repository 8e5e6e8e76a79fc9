/* gigs_hip.h -- C ABI of libgigs_hip.so, the MI355X (gfx950) implementation of the GI-GS
 * rasterizer hot path.
 *
 * Every entry point replaces one static method of `CudaRasterizer::Rasterizer`
 * (reference: submodules/diff-gaussian-rasterization/cuda_rasterizer/rasterizer.h:20-199,
 * "R/" below) or one kornia call the reference makes inside the operator.  All pointers
 * are DEVICE pointers owned by the caller unless a parameter says "host".  Nothing is
 * allocated or freed by the library; scratch memory is requested from the caller through
 * `gigs_alloc_fn` callbacks, the C form of the reference's
 * `std::function<char*(size_t)>` resize functors (R/rasterize_points.cu:31-37).
 *
 * Conventions
 *   - return value: >= 0 on success (gigs_forward returns num_rendered), < 0 on error;
 *     `gigs_last_error()` then returns a message (thread-local, host memory).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  The reference
 *     launches on the legacy default stream; the stream argument is the only addition.
 *   - image planes are planar CHW fp32 (R/cuda_rasterizer/forward.cu:608-610);
 *     `viewmatrix` / `projmatrix` are the 16 floats of the row-vector matrices the
 *     reference passes (scene/cameras.py:75-85).
 *   - optional inputs (shs / colors_precomp, scales+rotations / cov3D_precomp) are NULL
 *     when absent, like the null data_ptr of the reference's empty tensors
 *     (R/diff_gaussian_rasterization/__init__.py:435-445).
 */
#ifndef GIGS_HIP_H_
#define GIGS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GIGS_OK 0
#define GIGS_ERR_INVALID (-1)  /* bad argument (shape, null pointer, non-RGB without colours) */
#define GIGS_ERR_HIP (-2)      /* a HIP call or kernel failed; see gigs_last_error()           */
#define GIGS_ERR_ALLOC (-3)    /* an allocation callback returned NULL                        */

/* Replaces std::function<char*(size_t)> (R/rasterize_points.cu:31-37): must return a device
 * pointer to at least `nbytes` bytes that stays valid until the matching backward has run. */
typedef char* (*gigs_alloc_fn)(size_t nbytes, void* user);

const char* gigs_last_error(void);
/* "gfx950" -- the only architecture the code objects are built for. */
const char* gigs_build_arch(void);

/* ---- contexts: per-instance state -----------------------------------------------------------------
 * The reference's rasterizer is a set of stateless static methods (R/cuda_rasterizer/rasterizer.h:20-199) that
 * all run on the legacy default stream.  This library adds streams, an asynchronous binning mode, a
 * scheduling event and a number of tuning / diagnostic switches -- and keeps ALL of that in a context the
 * caller owns, so that two rasterizer instances (or two streams) of one process do not see each other:
 * every entry point that reads such state takes a `gigs_ctx*` first.  NULL = the default context: the
 * options below as the environment gave them when the library was first used (parsed ONCE, immutable
 * afterwards), no asynchronous binning, no event.  Calls only READ their context, so any number of threads
 * and streams may use one concurrently; the gigs_ctx_set_* functions must not race with calls that use it.
 * Different contexts are independent (what the library itself caches process-wide -- ray tables, texel
 * tables, temp-storage sizes -- is keyed by its inputs and never modified once built).
 * The in-library profile session (gigs_profile_begin/end, a bench.py diagnostic) is the one process-wide
 * facility left. */
typedef struct gigs_ctx gigs_ctx;
typedef struct gigs_options {
  int struct_bytes;     /* sizeof(gigs_options): set by the caller (ABI growth) */
  int binning_legacy;   /* 0 (default) tile-bucketed binning; 1 scan / duplicate / global radix sort / tile ranges, the
                           reference's structure (identical keys, point_list, ranges).        env GIGS_BINNING=legacy */
  int bucket_max_mean;  /* mean instances per tile above which a scene counts as dense (2500). env GIGS_BUCKET_MAX_MEAN */
  int long_lists;       /* -1 (default) by density, 0 / 1 forbid / force the long-list partition.  env GIGS_LONG_LISTS */
  int bucket_target;    /* keys per bucket of that partition (1536).                            env GIGS_BUCKET_TARGET */
  int bin_bands;        /* passes of the by-tile scatter over bands of tile rows: 0 (default) = 4 for dense scenes, else 1;
                           same keys, point_list, ranges.                                          env GIGS_BIN_BANDS */
  int blend_cull;       /* 1 (default); 0 = blend forward without the quadrant cull (same bits). env GIGS_BLEND_CULL */
  int pre_bwd_sh_skip;  /* 1 (default); 0 = the preprocess backward evaluates every chain.   env GIGS_PRE_BWD_SH_SKIP */
  int gi_march;         /* SSAO / SSR march: 0 exact (the oracle's pixel choices bit for bit), 4 proj (default); no other
                           value is valid.                                                   env GIGS_GI_MARCH=exact|proj */
  int gi_cert;          /* 1 (default) coarse-depth certification in front of the proj march (same bits). env GIGS_GI_CERT */
  int gi_interleave;    /* 1 (default) interleaved ray pairs per wave, 0 contiguous quarters.     env GIGS_GI_INTERLEAVE */
  int gi_tile_log2w;    /* pixel rectangle of a march workgroup, 2^k x 64/2^k, k = 0..6 (3).      env GIGS_GI_TILE_LOG2W */
  int gi_zero_rays;     /* 0 (default) the zero-weight rays (theta = 0: 32 of 512 at delta 0.0625) are not marched -- their
                           contributions are exact zeros; 1 = marched all the same (same bits).   env GIGS_GI_ZERO_RAYS */
  int spec_max8;        /* largest mean GGX window served by 8-lane groups (128).                   env GIGS_SPEC_MAX8 */
  int spec_max16;       /* ... by 16-lane groups (1500).                                            env GIGS_SPEC_MAX16 */
  int shade_lds_floats; /* LDS accumulator budget of the shade backward in floats (30720).    env GIGS_SHADE_LDS_FLOATS */
  int shade_bwd_blocks; /* its persistent workgroups, 0 (default) = one per CU.               env GIGS_SHADE_BWD_BLOCKS */
  int shade_bwd_rows;   /* 0 (default) its pixels in 32x32 tiles of 8x8-pixel waves, one add per distinct texel of a
                           wave into the global light levels; 1 = row-major chunks, adds pre-summed in 16-lane runs
                           (every per-pixel output the same bits).                         env GIGS_SHADE_BWD_ROWS */
  int spec_sparse;      /* 1 (default): gigs_specular_cubemap_multi_bwd_sparse scatters the levels whose incoming gradient
                           has few nonzero texels; 0 = it launches what gigs_specular_cubemap_multi_w launches. env GIGS_SPEC_SPARSE */
  int spec_sparse_permille; /* capacity of a level's list of nonzero texels in thousandths of its texels, 0..1000 (100): a
                           level with more nonzero texels is gathered.                     env GIGS_SPEC_SPARSE_PERMILLE */
} gigs_options;
/* A new context holds a copy of the default options.  Destroying a context frees host memory only; work queued
 * with it may still be running. */
gigs_ctx* gigs_ctx_create(void);
void gigs_ctx_destroy(gigs_ctx* ctx);
/* out->struct_bytes must be set by the caller; ctx == NULL reads the defaults.  set: values outside their range are
 * rejected (GIGS_ERR_INVALID) and nothing changes; ctx must not be NULL (the default context is immutable). */
int gigs_ctx_get_options(const gigs_ctx* ctx, gigs_options* out);
int gigs_ctx_set_options(gigs_ctx* ctx, const gigs_options* in);

/* Scratch sizes: required<GeometryState>(P), required<ImageState>(N), required<BinningState>(R)
 * (R/cuda_rasterizer/rasterizer_impl.h:67-73).  Need a visible GPU (rocPRIM temp-storage
 * queries). Return 0 and set the error string on failure. */
size_t gigs_required_geom(int P);
size_t gigs_required_image(int width, int height);
size_t gigs_required_binning(int num_rendered);

/* Rasterizer::forward (R/cuda_rasterizer/rasterizer.h:24-63, rasterizer_impl.cu:486-672).
 * Runs preprocess -> scan -> (one 4-byte D2H read of num_rendered) -> duplicate -> radix sort
 * -> tile ranges -> G-buffer blend.  `background` is 3 floats.  `radii` may be NULL.
 * Every pixel of every output plane and every radii[i] is written when P > 0; when P == 0 nothing
 * is launched and the caller's (zero) initialisation stays. */
int gigs_forward(gigs_ctx* ctx, gigs_alloc_fn geometryBuffer, void* geom_user, gigs_alloc_fn binningBuffer,
                 void* binning_user, gigs_alloc_fn imageBuffer, void* image_user, int P, int D, int M,
                 const float* background, int width, int height, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* opacities,
                 const float* normal, const float* albedo, const float* roughness,
                 const float* metallic, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                 int prefiltered, int argmax_depth, int inference, float* out_color,
                 float* out_opacity, float* out_depth, float* out_normal, float* out_normal_view,
                 float* out_pos, float* out_albedo, float* out_roughness, float* out_metallic,
                 int* radii, int debug, void* stream);

/* Rasterizer::backward (rasterizer.h:103-150, rasterizer_impl.cu:676-803).  Every element of every
 * dL_d* output is written (culled Gaussians get zeros), so the caller need not zero-initialise them
 * as the reference binding does (R/rasterize_points.cu:299-312); dL_dconic [P,2,2] and dL_ddepth [P]
 * are the two scratch gradients the reference allocates but does not return: either may be NULL (not
 * written).  Any of the seven incoming dL_dpix_* planes may be NULL = an all-zero gradient (an output
 * the loss does not use). */
int gigs_backward(gigs_ctx* ctx, int P, int D, int M, int R, const float* background, int width, int height,
                  const float* means3D, const float* shs, const float* colors_precomp,
                  const float* normal, const float* albedo, const float* roughness,
                  const float* metallic, const float* scales, const float* rotations,
                  const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                  const float* cam_pos, const int* radii, float scale_modifier, float tan_fovx,
                  float tan_fovy, char* geom_buffer, char* binning_buffer, char* image_buffer,
                  const float* dL_dpix_depth, const float* dL_dpix, const float* dL_dpix_opacity,
                  const float* dL_dpix_normal, const float* dL_dpix_albedo,
                  const float* dL_dpix_roughness, const float* dL_dpix_metallic, float* dL_dmean2D,
                  float* dL_dconic, float* dL_ddepth, float* dL_dopacity, float* dL_dnormal,
                  float* dL_dalbedo, float* dL_droughness, float* dL_dmetallic, float* dL_dcolor,
                  float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                  float* dL_drot, int debug, void* stream);

/* Rasterizer::markVisible (rasterizer.h:24-29 / rasterizer_impl.cu:141-153); present = bool[P]. */
int gigs_mark_visible(int P, const float* means3D, const float* viewmatrix,
                      const float* projmatrix, uint8_t* present, void* stream);

/* Rasterizer::depthToNormal (rasterizer_impl.cu:201-220 -> forward.cu:914-1032).  Every pixel of
 * `normal` and `depth_pos` ([3,H,W]) is written (zeros where the reference leaves its zero fill). */
int gigs_depth_to_normal(int width, int height, float focal_x, float focal_y,
                         const float* viewmatrix, const float* depth, float* normal,
                         float* depth_pos, void* stream);

/* Rasterizer::SSAO (rasterizer_impl.cu:222-253 -> forward.cu:635-724). occlusion = [1,H,W], fully written. */
/* The chain GaussianRasterizer.forward runs between the blend and SSAO (R/diff_gaussian_rasterization/__init__.py:475-517)
 * as ONE launch: normal_from_depth = bilateral3x3(depth_to_normal(median3x3(depth)).normal, sigma_color, sigma_x, sigma_y),
 * depth_pos_filter = median3x3(depth_to_normal(median3x3(depth)).pos).  Bit-identical to calling gigs_median3x3,
 * gigs_depth_to_normal, gigs_bilateral3x3 and gigs_median3x3 in turn (gigs-hip extension; depth [1,H,W], outputs [3,H,W]). */
int gigs_derive_normal(int width, int height, float focal_x, float focal_y, const float* viewmatrix, const float* depth,
                       float sigma_color, float sigma_x, float sigma_y, float* normal_from_depth, float* depth_pos_filter,
                       void* stream);
int gigs_ssao(int width, int height, float focal_x, float focal_y, float radius, float bias,
              float thick, float delta, int step, int start, const float* normal_view,
              const float* pos, float* occlusion, void* stream);

/* Rasterizer::SSR (rasterizer_impl.cu:255-298 -> forward.cu:726-909). color, abd = [3,H,W]. */
int gigs_ssr(int width, int height, float focal_x, float focal_y, float radius, float bias,
             float thick, float delta, int step, int start, const float* normal_view,
             const float* pos, const float* rgb, const float* albedo, const float* roughness,
             const float* metallic, const float* F0, float* color, float* abd, void* stream);

/* The same two passes with a caller-owned scratch buffer of gigs_gi_scratch_bytes(width, height) bytes (gigs-hip
 * extension; may be NULL = identical to the plain entries).  With it the default march first builds a min/max table
 * of the position plane's z over 16..64-pixel blocks there and skips, conservatively, the z-plane lookups of samples
 * that cannot hit: bit-identical outputs, ~92 % fewer gathers on the bench view.  The buffer is
 * only used during the call's kernels (stream-ordered).  `ctx` selects the march (gigs_options.gi_*; NULL = defaults);
 * gigs_ssao / gigs_ssr are these with ctx = NULL and scratch = NULL. */
size_t gigs_gi_scratch_bytes(int width, int height);
int gigs_ssao_ex(gigs_ctx* ctx, int width, int height, float focal_x, float focal_y, float radius, float bias,
                 float thick, float delta, int step, int start, const float* normal_view,
                 const float* pos, float* occlusion, void* scratch, void* stream);
int gigs_ssr_ex(gigs_ctx* ctx, int width, int height, float focal_x, float focal_y, float radius, float bias,
                float thick, float delta, int step, int start, const float* normal_view,
                const float* pos, const float* rgb, const float* albedo, const float* roughness,
                const float* metallic, const float* F0, float* color, float* abd, void* scratch, void* stream);

/* The hit list of the indirect-light march (gigs-hip extension; frozen-geometry reuse).  WHICH pixel each ray of each pixel
 * hits depends on normals and positions only (forward.cu:796-829), not on the radiance gathered there, so a view whose geometry
 * does not change marches once and gathers afterwards.  gigs_ssr_hits is gigs_ssr_ex (same outputs) that additionally,
 *   mode 1: writes counts[4 * pixel + w] = the number of hits of pixel's rays handled by wave w of its workgroup (u32 [4 N]);
 *   mode 2: given offsets = the exclusive prefix of those counts (u32 [4 N + 1]), writes the hits in march order as
 *           {hit pixel, ray index} pairs (2 x u32 each) at offsets[...]; pairs beyond `capacity` are dropped -- compare
 *           offsets[4 N] with it.
 * gigs_ssr_apply evaluates color / abd from such a list: per pixel the four sequences are summed in order, combined as the
 * march combines its four waves, and the same tail applied -- the march's outputs bit for bit while normals / positions are the
 * recorded ones.  Recorded by the default march only (gigs_options.gi_march = 4). */
int gigs_ssr_hits(gigs_ctx* ctx, int width, int height, float focal_x, float focal_y, float radius, float bias, float thick,
                  float delta, int step, int start, const float* normal_view, const float* pos, const float* rgb,
                  const float* albedo, const float* roughness, const float* metallic, const float* F0, float* color, float* abd,
                  int mode, unsigned* counts, const unsigned* offsets, void* entries, unsigned capacity, void* scratch,
                  void* stream);
int gigs_ssr_apply(int width, int height, float delta, const unsigned* offsets, const void* entries, const float* normal_view,
                   const float* pos, const float* rgb, const float* albedo, const float* metallic, const float* F0,
                   float* color, float* abd, void* stream);

/* The indirect-light march over K radiance planes (gigs-hip extension; relighting one view under K environment maps).
 * rgb, color and abd are [K,3,H,W]; the hits depend on normal_view / pos only, so every pixel marches once per group of up
 * to GIGS_SSR_LIGHTS_PER_MARCH planes and gathers them all (ceil(K / that) marches; the certification table is built once).
 * color[k] and abd[k] equal gigs_ssr_ex with rgb = rgb[k] bit for bit, in every march mode (abd = the gathered irradiance
 * times kD before the albedo: it depends on the light).  1 <= K <= GIGS_MAX_LIGHTS, else GIGS_ERR_INVALID. */
#define GIGS_MAX_LIGHTS 16
#define GIGS_SSR_LIGHTS_PER_MARCH 4
int gigs_ssr_multi(gigs_ctx* ctx, int n_lights, int width, int height, float focal_x, float focal_y, float radius, float bias,
                   float thick, float delta, int step, int start, const float* normal_view, const float* pos, const float* rgb,
                   const float* albedo, const float* roughness, const float* metallic, const float* F0, float* color,
                   float* abd, void* scratch, void* stream);

/* gigs_ssr_apply for K radiance planes (gigs-hip extension; one view under many lights, relight.TurntableRelighter): rgb,
 * color and abd are [K,3,H,W], everything else as in gigs_ssr_apply.  The list is walked once per pass of up to 8 planes:
 * the pass first packs its planes pixel-major into `scratch` (gigs_ssr_apply_multi_scratch_bytes(K, width, height) bytes,
 * 16-byte aligned, used during the call's kernels only; may be NULL for K = 1), so that a hit is a few adjacent 16-byte
 * loads for all its lights; each hit entry and its ray weights are read once per pass, and every light keeps its own sums
 * in gigs_ssr_apply's order.  color[k] / abd[k] equal gigs_ssr_apply with rgb = rgb[k] bit for bit, hence gigs_ssr_ex /
 * gigs_ssr_multi for the geometry the list was recorded with.  `offsets` must be 16-byte aligned and the list complete
 * (offsets[4 N] <= the capacity it was filled with: the caller's check).  1 <= K <= GIGS_MAX_LIGHTS, else GIGS_ERR_INVALID. */
size_t gigs_ssr_apply_multi_scratch_bytes(int n_lights, int width, int height);
int gigs_ssr_apply_multi(int n_lights, int width, int height, float delta, const unsigned* offsets, const void* entries,
                         const float* normal_view, const float* pos, const float* rgb, const float* albedo,
                         const float* metallic, const float* F0, float* color, float* abd, void* scratch, void* stream);

/* kornia.filters.median_blur(x[None], (3,3))[0] as called at
 * R/diff_gaussian_rasterization/__init__.py:478, 504 (zero padding, NaN-propagating). */
int gigs_median3x3(int channels, int height, int width, const float* in, float* out, void* stream);
/* Backward of the above: routes each output gradient to the tap that was selected. */
int gigs_median3x3_backward(int channels, int height, int width, const float* in,
                            const float* grad_out, float* grad_in, void* stream);

/* kornia.filters.bilateral_blur(x[None], (3,3), sigma_color, (sigma_y, sigma_x))[0]
 * (…/__init__.py:491; reflect border, L1 colour distance). */
int gigs_bilateral3x3(int channels, int height, int width, float sigma_color, float sigma_x,
                      float sigma_y, const float* in, float* out, void* stream);

/* ---- deferred shade and cubemap light (pbr/shade.py, pbr/light.py, pbr/renderutils) ----------
 * Cubemaps are [6, res, res, 3] fp32 (NHWC as in the reference); HWC image tensors as passed to
 * pbr_shading.  Sampling rule of the texture lookups (the reference uses nvdiffrast dr.texture,
 * third party, parity unpinned): cube face/(u,v) selection by the dominant axis with the face
 * orientations of pbr/light.py:40-52; bilinear taps at (uv * size - 0.5); a tap that leaves a face
 * is taken from the neighbouring face, the single missing tap at a cube corner is dropped and the
 * weights renormalised; 2-D lookups clamp tap indices; the mip blend uses
 * level = clamp(mip_level_bias, 0, L-1) between floor(level) and floor(level)+1. */

/* diffuse_cubemap_fwd / _bwd (pbr/renderutils/c_src/torch_bindings.cpp:740-795 -> cubemap.cu:110-169).
 * The backward is a gather over the same weights; grad_cubemap is fully overwritten. */
int gigs_diffuse_cubemap_fwd(int res, const float* cubemap, float* out, void* stream);
int gigs_diffuse_cubemap_bwd(int res, const float* grad_out, float* grad_cubemap, void* stream);
/* specular_bounds (torch_bindings.cpp:797-822 -> cubemap.cu:181-244): bounds = [6,res,res,24]. */
int gigs_specular_bounds(int res, float costheta_cutoff, float* bounds, void* stream);
/* specular_cubemap_fwd / _bwd (torch_bindings.cpp:824-890 -> cubemap.cu:246-350).  out and grad_out
 * are [6,res,res,4] (rgb, weight sum); grad_cubemap [6,res,res,3] is fully overwritten.  bounds = what
 * gigs_specular_bounds gives for (res, costheta_cutoff).  The backward is the transpose of the forward: a gather
 * over the texel's own window where the accepted set of (res, costheta_cutoff) is symmetric, else a scatter over
 * each output's window with float atomics (the bounds' tile cull drops in-cone texels at coarse resolutions).  The
 * first backward of a (device, res, costheta_cutoff) decides which and synchronises the stream once. */
int gigs_specular_cubemap_fwd(int res, const float* cubemap, const float* bounds, float roughness,
                              float costheta_cutoff, float* out, void* stream);
int gigs_specular_cubemap_bwd(int res, const float* bounds, const float* grad_out, float roughness,
                              float costheta_cutoff, float* grad_cubemap, void* stream);
/* The same filter through a cached weight table (an MI355X-specific addition, no reference
 * counterpart): the pair weights depend only on (res, roughness, cutoff), so they are computed once
 * into `weights` and the per-step filter becomes a streaming pass.  offsets = uint32 [6*res*res*6]
 * exclusive prefix sums of the per-(texel, face) AABB areas of `bounds`; weights holds that many floats
 * (+ the last area).  swap_roles = 0 builds the table the forward reads, 1 the one the backward reads
 * (the NDF argument V.H is evaluated with the reference's operand roles in both, so results are
 * bit-identical to the table-free entry points up to summation order). */
int gigs_specular_weights(int res, const float* bounds, const uint32_t* offsets, float roughness,
                          float costheta_cutoff, int swap_roles, float* weights, void* stream);
/* out_weights[o][i] = weights[o][i] / texel_divisor[texel i of o's window] (negative markers kept), texel_divisor
 * [6,res,res].  Applied to the role-swapped table with the forward's weight sums it yields a table whose gather of the
 * incoming gradient IS the backward of the normalised filter (no separate division by wsum). */
int gigs_specular_weights_divide(int res, const float* bounds, const uint32_t* offsets, const float* weights,
                                 const float* texel_divisor, float* out_weights, void* stream);
/* wsum_out == NULL: out = [6,res,res,4] (rgb, weight sum) like the table-free entry point;
 * wsum_out != NULL: out = [6,res,res,3] = rgb / wsum (the division of ops.py:458 folded in) and the
 * weight sums go to wsum_out [6,res,res].  grad_is_rgb: grad_out is [6,res,res,3] (already divided
 * by wsum by the caller) instead of [6,res,res,4].  avg_window = table length / (6 res^2), the mean
 * number of candidates per texel: a scheduling hint only (lanes per texel), 0 = unknown. */
int gigs_specular_cubemap_fwd_w(gigs_ctx* ctx, int res, const float* cubemap, const float* bounds, const uint32_t* offsets,
                                const float* weights, int avg_window, float* out, float* wsum_out, void* stream);
int gigs_specular_cubemap_bwd_w(gigs_ctx* ctx, int res, const float* bounds, const uint32_t* offsets,
                                const float* weights_swapped, int avg_window, const float* grad_out,
                                int grad_is_rgb, float* grad_cubemap, void* stream);
/* 1 if the accepted set of (res, costheta_cutoff) is symmetric -- every pair (o, i) with i inside o's AABB and inside the
 * cone also has o inside i's AABB --, 0 if not, < 0 on error.  Decided once per (device, res, costheta_cutoff) from
 * gigs_specular_bounds' own output and cached; the first query synchronises the stream, so ask where the bounds and tables
 * are built.  The role-swapped tables (gigs_specular_cubemap_bwd_w, the backward of gigs_specular_cubemap_multi_w and the
 * gathered levels of gigs_specular_cubemap_multi_bwd_sparse) are the transpose of the forward ONLY for a symmetric level;
 * the backward of any other level is gigs_specular_cubemap_bwd_scatter_w (pbr.renderutils.ops routes them). */
int gigs_specular_window_symmetric(int res, float costheta_cutoff, void* stream);
/* The backward from the FORWARD table in scatter form, for any level: grad_cubemap[i] = sum over the outputs o whose run
 * holds i with a weight >= 0 of (w / wsum[o]) * grad_out[o].rgb (wsum = the forward's weight sums [6,res,res]: the backward
 * of the normalised filter) or, with wsum == NULL, of w * grad_out[o].rgb.  grad_out is [6,res,res,3] (grad_is_rgb != 0) or
 * [6,res,res,4].  grad_cubemap is cleared, then added into with float atomics: the order of the additions is not fixed. */
int gigs_specular_cubemap_bwd_scatter_w(int res, const float* bounds, const uint32_t* offsets, const float* weights_fwd,
                                        const float* wsum, const float* grad_out, int grad_is_rgb, float* grad_cubemap,
                                        void* stream);

/* The table-driven GGX filter of ALL levels of a light in one launch (gigs-hip extension): the levels of
 * CubemapLight.build_mips (pbr/light.py:166-170) are independent of each other, so their texels share one grid instead of
 * one dependent launch per level.  `levels` is a HOST array; per level the arguments of gigs_specular_cubemap_fwd_w
 * (backward = 0: src = the level's mip, dst = rgb / wsum [6,res,res,3], wsum [6,res,res] required) or of
 * gigs_specular_cubemap_bwd_w with grad_is_rgb = 1 (backward = 1: src = the incoming gradient, weights = the role-swapped
 * table already divided by the forward's weight sums, dst = the gradient w.r.t. the mip, wsum unused). */
typedef struct gigs_spec_level {
  int res, avg_window;
  const float* src;
  const float* bounds;
  const uint32_t* offsets;
  const float* weights;
  float* dst;
  float* wsum;
} gigs_spec_level;
int gigs_specular_cubemap_multi_w(gigs_ctx* ctx, int n_levels, const gigs_spec_level* levels, int backward, void* stream);
/* The backward of the above (levels as for backward = 1) for gradients that are mostly exact zeros, which is what the shade
 * backward hands the fine levels: it zero-fills them and adds into the sampled texels only.  Three launches, every decision
 * taken on the device (fixed grids, no read-back: capturable in a graph and replayable with other gradients):
 *   census   one pass over every level's src: zero-fills dst, counts the texels with a channel != 0 (NaN counts, -0 does
 *            not) and lists their indices, up to the level's capacity = gigs_spec_sparse_capacity(ctx, res);
 *   apply    one launch for every level.  A level whose count is within its capacity is SPARSE: the products
 *            (w / wsum[o]) * src[o], w >= 0 from the listed texel o's run of the FORWARD table weights_fwd[level] (the
 *            products of the gather's pre-divided table), are summed on chip by the workgroups that own 16 x 16 tiles
 *            of dst, or, for a level whose mean window holds at most 256 candidates, added into dst with float atomics
 *            by one wave per listed texel.  The other levels are gathered by the workgroups of
 *            gigs_specular_cubemap_multi_w and get the same bits as from that call;
 *   finish   one wave: writes the report below and clears the working counters.
 * wsum[level] = the forward's weight sums [6,res,res].  state: GIGS_SPEC_SPARSE_STATE_INTS device ints, zero before the
 * first call and owned by one stream at a time; after a call state[8 + l] = 1 if level l took a sparse path, 0 if gathered, and
 * state[16 + l] = its count of nonzero texels (state[0..7] are the working counters: the last kernel clears them for the
 * next call).  lists: device ints, the levels' capacities in level order.  With gigs_options.spec_sparse = 0 the call is
 * gigs_specular_cubemap_multi_w(backward = 1) and touches neither state nor lists. */
#define GIGS_SPEC_SPARSE_STATE_INTS 32
int gigs_spec_sparse_capacity(const gigs_ctx* ctx, int res);
int gigs_specular_cubemap_multi_bwd_sparse(gigs_ctx* ctx, int n_levels, const gigs_spec_level* levels,
                                           const float* const* weights_fwd, const float* const* wsum, int* state,
                                           int* lists, void* stream);
/* The forward of gigs_specular_cubemap_multi_w for a caller that shades ONE view with the light it has just built (a
 * training step): only the texels that view's shade reads are filtered.  Two calls, no read-back (capturable):
 *   gigs_spec_tap_census   marks, per pixel, the (up to 8) texels the specular lookup of the shade reads: the level
 *            pair of the pixel's roughness (raw * rough_scale + rough_bias) and the four bilinear taps of the reflected
 *            direction in each, through the very function the shade kernels sample through.  The shading normal is either
 *            `normals` ([H,W,3], or [3,H,W] with planar = 1) or derived from normal_map [3,H,W] and viewmatrix exactly as
 *            gigs_shade_fwd_post derives it (normals null).  The shade kernels sample the levels for EVERY pixel, inside
 *            their mask or not, so every pixel marks; `mask` ([H,W] bytes, with `normals` only, null = every pixel) is for
 *            a caller that will not shade the pixels it leaves out -- a shade over them reads texels that are not listed.
 *            needed[l]: [6,res_l,res_l,3] floats, ZERO before the call, or null for a level that is not listed; channel 0
 *            of a marked texel becomes 1.  view_dirs [H,W,3], roughness [H,W].
 *   gigs_specular_cubemap_multi_fwd_sparse   for the given levels (as for gigs_specular_cubemap_multi_w, backward = 0):
 *            lists the marked texels of needed[l] (and clears the marks: the arrays are zero again afterwards), then filters
 *            in ONE launch the listed texels of every level whose count is within capacities[l] -- each gets the bits the
 *            dense launch gives it; dst and wsum of the other texels are NOT written -- and every texel of a level whose
 *            count exceeds its capacity.  state / lists as for gigs_specular_cubemap_multi_bwd_sparse (a state of its own:
 *            state[8 + l] = 1 listed, 0 dense; state[16 + l] = texels marked; lists holds sum(capacities) ints).
 * Texels that are not listed keep whatever dst held: the result is a light for this view's shade only. */
int gigs_spec_tap_census(gigs_ctx* ctx, int H, int W, const float* normals, int planar, const float* normal_map,
                         const float* viewmatrix, const float* view_dirs, const float* roughness, const uint8_t* mask,
                         float rough_scale, float rough_bias, int n_levels, const int* spec_res, float* const* needed,
                         void* stream);
int gigs_specular_cubemap_multi_fwd_sparse(gigs_ctx* ctx, int n_levels, const gigs_spec_level* levels, float* const* needed,
                                           const int* capacities, int* state, int* lists, void* stream);
/* cubemap_mip (pbr/light.py:54-79): forward 2x2 average pool [6,2r,2r,C] -> [6,r,r,C]; backward =
 * bilinear cube lookup of 0.25*dout at every fine texel direction, dout [6,r,r,3] -> din [6,2r,2r,3]. */
int gigs_cubemap_mip_fwd(int res_out, int channels, const float* in, float* out, void* stream);
int gigs_cubemap_mip_bwd(int res_out, const float* dout, float* din, void* stream);
/* din = add + the above (add [6,2r,2r,3]: the gradient the fine level receives from its other consumer, so that the
 * chain base <- mip1 <- ... <- mipN is walked back without separate accumulation passes). */
int gigs_cubemap_mip_bwd_add(int res_out, const float* dout, const float* add, float* din, void* stream);
/* the same with a second gradient of the coarse level: din = add + lookup(0.25 * (dout + dout2)); dout2 and add may be
 * NULL.  (The coarsest level feeds the GGX filter and the diffuse filter, the base the GGX filter and the chain.) */
int gigs_cubemap_mip_bwd_add2(int res_out, const float* dout, const float* dout2, const float* add, float* din, void* stream);

/* pbr_shading (pbr/shade.py:108-241) fused into one kernel.  normals/view_dirs/albedo [H,W,3],
 * roughness/occlusion/metallic [H,W,1] (occlusion, metallic, background may be NULL), mask = bool
 * [H,W,1]; diffuse = light.diffuse [6,dres,dres,3]; spec = HOST array of n_levels device pointers
 * (light.specular), spec_res their resolutions (host); lut = BRDF LUT [lut_h, lut_w, 2].
 * Outputs [H,W,3]: render_rgb, diffuse_rgb, specular_rgb, diffuse_light (the result dict). */
int gigs_shade_fwd(int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                   const float* roughness, const uint8_t* mask, const float* occlusion,
                   const float* metallic, const float* background, const float* diffuse, int diffuse_res,
                   int n_levels, const float* const* spec, const int* spec_res, const float* lut,
                   int lut_w, int lut_h, int tone, int gamma, float* render_rgb, float* diffuse_rgb,
                   float* specular_rgb, float* diffuse_light, void* stream);
/* Backward of the above.  g_* are gradients w.r.t. the four outputs (any may be NULL = zero).
 * d_albedo [H,W,3], d_roughness [H,W,1], d_metallic [H,W,1] (NULL when metallic is NULL) are
 * overwritten; d_diffuse and d_spec[i] (host array of device pointers, entries may be NULL) are
 * ACCUMULATED with float atomics and must be zero-initialised by the caller. */
int gigs_shade_bwd(int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                   const float* roughness, const uint8_t* mask, const float* occlusion,
                   const float* metallic, const float* diffuse, int diffuse_res, int n_levels,
                   const float* const* spec, const int* spec_res, const float* lut, int lut_w, int lut_h,
                   int tone, int gamma, const float* g_render, const float* g_diffuse_rgb,
                   const float* g_specular_rgb, const float* g_diffuse_light, float* d_albedo,
                   float* d_roughness, float* d_metallic, float* d_diffuse, float* const* d_spec,
                   void* stream);

/* Stage-2 fusion hooks for the two shade entry points (gigs-hip extension; NULL = the plain operator).
 * They fold the tensor glue train.py wraps around pbr_shading into the same kernels:
 *   planar         1: normals, albedo and every [H,W,3] output / gradient are [3,H,W] planes, i.e. the
 *                  rasterizer's own layout (no permute + copy);  view_dirs stays [H,W,3]
 *   rough_scale/bias  roughness = raw * scale + bias (train.py:293-295); d_roughness is w.r.t. raw
 *   forward extras (may be NULL, output layout): out_F0 = (1-m)*0.04 + albedo*m (train.py:352-356),
 *                  out_linear = srgb_to_linear(render_rgb) (train.py:70-81), out_roughness [H,W]
 *   backward extras (may be NULL): d_albedo += g_albedo_mul_a * g_albedo_mul_b (Gaussian_SSR's closed-form
 *                  backward grad_out * abd, R/diff_gaussian_rasterization/__init__.py:671-673);
 *                  g_roughness_add / g_metallic_add [H,W] are added to the roughness (remapped) / metallic
 *                  gradients (the lamb regulariser, train.py:401-402);
 *                  g_scale (device scalar, NULL = 1): g_render and g_albedo_mul_a are gradients for a UNIT upstream
 *                  gradient (gigs_stage2_loss_fwd_grad writes them in the forward) and are multiplied by it here;
 *                  lamb_mask [H,W] + lamb_acc4 (gigs_stage2_loss_fwd's acc4): the lamb regulariser's gradients
 *                  -/+ mask / acc4[3] * 0.001 * g_scale are formed here instead of being read from g_*_add.
 * With ext != NULL diffuse_rgb / specular_rgb / diffuse_light may be NULL (not written). */
typedef struct gigs_shade_ext {
  int planar;
  float rough_scale, rough_bias;
  float *out_F0, *out_linear, *out_roughness;
  const float *g_albedo_mul_a, *g_albedo_mul_b, *g_roughness_add, *g_metallic_add;
  const float *g_scale, *lamb_mask, *lamb_acc4;
} gigs_shade_ext;
int gigs_shade_fwd_ex(gigs_ctx* ctx, int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                      const float* roughness, const uint8_t* mask, const float* occlusion,
                      const float* metallic, const float* background, const float* diffuse, int diffuse_res,
                      int n_levels, const float* const* spec, const int* spec_res, const float* lut,
                      int lut_w, int lut_h, int tone, int gamma, float* render_rgb, float* diffuse_rgb,
                      float* specular_rgb, float* diffuse_light, const gigs_shade_ext* ext, void* stream);
/* gigs_gbuffer_post followed by gigs_shade_fwd_ex (planar layout: ext->planar must be 1; no background, render_rgb and the
 * ext outputs only) as ONE launch (gigs-hip extension; the fused stage-2 node): a workgroup normalises its tile of
 * normal_map / out_normal_view once into LDS, forms the medians, the rotation and the mask from there, stores
 * normals_view, normal_mask (u8, required), normal_mask_f (may be NULL) and out_normal_view_filtered as
 * gigs_gbuffer_post does, and shades each pixel from the normal and the mask it holds in registers.  Every output is bit
 * for bit that of the two calls. */
int gigs_shade_fwd_post(gigs_ctx* ctx, int H, int W, const float* normal_map, const float* out_normal_view,
                        const float* viewmatrix, float* normals_view, uint8_t* normal_mask, float* normal_mask_f,
                        float* out_normal_view_filtered, const float* view_dirs, const float* albedo,
                        const float* roughness, const float* occlusion, const float* metallic, const float* diffuse,
                        int diffuse_res, int n_levels, const float* const* spec, const int* spec_res, const float* lut,
                        int lut_w, int lut_h, int tone, int gamma, float* render_rgb, const gigs_shade_ext* ext,
                        void* stream);
/* gigs_shade_fwd_ex in the planar layout (ext->planar = 1, rough_scale 1, bias 0, no background) under K lights at once
 * (gigs-hip extension): diffuse[k] is light k's diffuse map, spec[k * n_levels + l] its level l; all lights share
 * diffuse_res, n_levels and spec_res.  The light-independent terms (vectors, cube taps, BRDF LUT, mip level, F0) are
 * computed once per pixel.  render_rgb[k] ([K,3,H,W]) and out_linear[k] (may be NULL) equal gigs_shade_fwd_ex with light
 * k bit for bit.  1 <= K <= GIGS_MAX_LIGHTS. */
int gigs_shade_fwd_multi(gigs_ctx* ctx, int n_lights, int H, int W, const float* normals, const float* view_dirs,
                         const float* albedo, const float* roughness, const uint8_t* mask, const float* occlusion,
                         const float* metallic, const float* const* diffuse, int diffuse_res, int n_levels,
                         const float* const* spec, const int* spec_res, const float* lut, int lut_w, int lut_h, int tone,
                         int gamma, float* render_rgb, float* out_linear, void* stream);
int gigs_shade_bwd_ex(gigs_ctx* ctx, int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                      const float* roughness, const uint8_t* mask, const float* occlusion,
                      const float* metallic, const float* diffuse, int diffuse_res, int n_levels,
                      const float* const* spec, const int* spec_res, const float* lut, int lut_w, int lut_h,
                      int tone, int gamma, const float* g_render, const float* g_diffuse_rgb,
                      const float* g_specular_rgb, const float* g_diffuse_light, float* d_albedo,
                      float* d_roughness, float* d_metallic, float* d_diffuse, float* const* d_spec,
                      const gigs_shade_ext* ext, void* stream);

/* The rest of the stage-2 tensor glue as single passes (gigs-hip extension; all planes [C,H,W] fp32).
 * gigs_gbuffer_post = gaussian_renderer/__init__.py:157-199 for normal_map and out_normal_view:
 *   normal_mask = (normal_map != 0).all(0)  (u8 and/or f32 copies, either may be NULL);
 *   normals_view = -(median3x3(normalize_where(normal_map)) @ viewmatrix[:3,:3]);
 *   out_normal_view_filtered = median3x3(normalize_where(out_normal_view)).  No gradient (detached in stage 2).
 * gigs_stage2_loss_fwd = train.py:382-402: render_rgb = render_direct + median3x3(linear_to_srgb(irr));
 *   loss = mean|render_rgb - gt| + 0.001 * (mean_mask(1 - roughness) + mean_mask(metallic)); acc4 is a
 *   scratch of GIGS_STAGE2_ACC_FLOATS floats whose first four receive {sum|.|, sum(1-r)m, sum(metallic m),
 *   sum m} (kept for the backward; the rest holds per-workgroup partial sums), render_rgb may be NULL.
 * gigs_stage2_loss_bwd: gradients of that loss (times *g_loss, NULL = 1) w.r.t. render_direct, irr (through the
 *   median's tap selection and the sRGB curve; overwritten), roughness and metallic [H,W]. */
#define GIGS_STAGE2_ACC_FLOATS (4 + 4 * 256)
int gigs_gbuffer_post(int height, int width, const float* normal_map, const float* out_normal_view,
                      const float* viewmatrix, float* normals_view, uint8_t* normal_mask, float* normal_mask_f,
                      float* out_normal_view_filtered, void* stream);
/* gigs_gbuffer_post_pad = the same post-processing with pad_normal=True (gaussian_renderer/__init__.py:157-199, as
 * render.py:212 calls it), one pass:
 *   opacity_out = opacity_map with < 0.004 -> 0, then > 1 - 0.004 -> 1 (may be NULL);
 *   normal_mask (u8 and/or f32, either may be NULL) from the UNPADDED normal_map;
 *   normal_world = median3x3(normalize_where(normal_map * a + (1 - a) * (0,0,1))) with a the thresholded opacity (may be
 *   NULL); normals_view = -(normal_world @ viewmatrix[:3,:3]); out_normal_view_filtered as gigs_gbuffer_post;
 *   normal_map_from_depth_out = normalize_where(all-zero pixels -> (0,0,1)) of normal_map_from_depth (may be NULL). */
int gigs_gbuffer_post_pad(int height, int width, const float* normal_map, const float* normal_map_from_depth,
                          const float* opacity_map, const float* out_normal_view, const float* viewmatrix,
                          uint8_t* normal_mask, float* normal_mask_f, float* normal_world, float* normals_view,
                          float* out_normal_view_filtered, float* normal_map_from_depth_out, float* opacity_out,
                          void* stream);
/* Stage 1 differentiates through the normal post-processing (train.py:327-328 use render()'s normal_map):
 * gigs_gbuffer_post_bwd = gradient of gigs_gbuffer_post's normals_view w.r.t. normal_map (rotation, the median's tap
 *   selection -- first tap in row-major order equal to the median, as gigs_median3x3_backward --, normalize_where);
 *   scratch3 is [3,H,W] floats of scratch (zeroed inside), g_normal_map [3,H,W] is overwritten.
 * gigs_normalize_mask = gaussian_renderer/__init__.py:157-163 for normal_map_from_depth: mask = (in != 0).all(0)
 *   (u8 [H,W], may be NULL), out = normalize_where(in). */
int gigs_gbuffer_post_bwd(int height, int width, const float* normal_map, const float* viewmatrix,
                          const float* g_normals_view, float* scratch3, float* g_normal_map, void* stream);
int gigs_normalize_mask(int height, int width, const float* in, float* out, uint8_t* mask, void* stream);
/* mask [H,W] (floats 0 / 1) = (in != 0).all(0) of in [3,H,W]: normal_mask of gaussian_renderer/__init__.py:158 as the
 * masked TV loss (train.py:116-142) weighs with it. */
int gigs_nonzero_mask(int height, int width, const float* in, float* mask, void* stream);
int gigs_stage2_loss_fwd(int height, int width, const float* render_direct, const float* irr_linear,
                         const float* gt_image, const float* normal_mask_f, const float* roughness,
                         const float* metallic, float* render_rgb, float* acc4, float* loss, void* stream);
int gigs_stage2_loss_bwd(int height, int width, const float* render_direct, const float* irr_linear,
                         const float* gt_image, const float* normal_mask_f, const float* acc4, const float* g_loss,
                         float* d_render_direct, float* d_irr_linear, float* d_roughness, float* d_metallic,
                         void* stream);
/* gigs_stage2_loss_fwd that also writes, in the same pass over the image (the backward kernel would convert the same
 * halo tiles and select the same medians again), the loss gradients w.r.t. render_direct and irr_linear for a unit
 * upstream gradient ([3,H,W] each; d_irr_linear_unit is zeroed inside and accumulated with atomics through the median's
 * tap selection).  gigs_shade_bwd_ex scales them (ext.g_scale) and forms the lamb terms (ext.lamb_*), so the stage-2
 * backward needs no loss kernel. */
int gigs_stage2_loss_fwd_grad(int height, int width, const float* render_direct, const float* irr_linear,
                              const float* gt_image, const float* normal_mask_f, const float* roughness,
                              const float* metallic, float* render_rgb, float* acc4, float* loss,
                              float* d_render_direct_unit, float* d_irr_linear_unit, void* stream);
/* gigs_stage2_loss_fwd_grad without global atomics and without cleared buffers (the fused stage-2 node's loss): the
 * median's gradient is GATHERED -- a workgroup evaluates median, sign and selected tap for its tile and the ring around
 * it, and each texel of d_irr_linear_unit adds, in a fixed order, the terms of the neighbours that selected it and is
 * written once (no zeroing; the same bits on every run).  render_rgb and d_render_direct_unit equal
 * gigs_stage2_loss_fwd_grad's bit for bit, d_irr_linear_unit up to the order of a texel's <= 9 terms.  The four sums go
 * through `scratch` (gigs_stage2_loss_gather_scratch_bytes(height, width) bytes, 16-byte aligned, need not be cleared),
 * one row of doubles per workgroup (64 x 8 pixels), added in a fixed order: they are accumulated in double throughout and
 * rounded to fp32 once.  acc4 here is the four totals only (4 floats), with gigs_stage2_loss_fwd's meaning; the loss is its
 * formula evaluated in double on those sums and rounded once (it can differ from gigs_stage2_loss_fwd_grad's in the last
 * bits: that entry adds in fp32 in the order its atomics arrive). */
size_t gigs_stage2_loss_gather_scratch_bytes(int height, int width);
int gigs_stage2_loss_gather(int height, int width, const float* render_direct, const float* irr_linear,
                            const float* gt_image, const float* normal_mask_f, const float* roughness,
                            const float* metallic, float* render_rgb, float* acc4, float* loss,
                            float* d_render_direct_unit, float* d_irr_linear_unit, void* scratch, size_t scratch_bytes,
                            void* stream);

/* dr.texture(cubemap[None], dirs[None], filter_mode="linear", boundary_mode="cube") (train.py:409-417, render.py:80,
 * relight.py:108) for n directions [n,3], sampled as the shade kernel samples light.diffuse (face by largest |axis|,
 * bilinear taps, taps beyond an edge come from the neighbouring face, the missing corner tap is dropped; the rule
 * documented at gigs_shade_fwd): out is [n,3], or three planes [3,n] if planar.
 * The backward accumulates into d_cubemap [6,res,res,3] (caller zeroes); directions get no gradient. */
int gigs_cube_texture_fwd(int res, const float* cubemap, int n, const float* dirs, float* out, int planar,
                          void* stream);
/* gigs_cube_texture_fwd (out [n,3]) with the texel coordinates and weights formed in double (gigs-hip extension; resampling
 * a light onto another cube grid, relight.rotate_light): the float lookup's coordinate error grows with res (half an ulp of
 * u * res - 0.5: 1.9e-6 texels at res 64, 7.6e-6 at 256) and a resample would write it into every texel.  Same faces and taps;
 * forward only. */
int gigs_cube_texture_fwd_precise(int res, const float* cubemap, int n, const float* dirs, float* out, void* stream);
/* latlong_to_cubemap (relight.py:92-111): cubemap [6,res_y,res_x,C] from an equirectangular map [lat_h,lat_w,C]:
 * texel direction = normalize(cube_to_dir(face, linspace(-1+1/res, 1-1/res))), tu = atan2(x,-z)/(2pi)+0.5,
 * tv = acos(clamp(y))/pi, then the 2D lookup dr.texture(latlong, (tu,tv), filter_mode="linear") -- nvdiffrast
 * (third party, absent): bilinear, texel centres at (i+0.5)/size, boundary_mode "wrap".  PARITY UNPINNED. */
int gigs_latlong_to_cubemap(int res_y, int res_x, int lat_h, int lat_w, int channels, const float* latlong,
                            float* cubemap, void* stream);
/* The same conversion for n_rot rotations of the map in one launch (gigs-hip extension; turntables): rotations is
 * [n_rot,3,3] row-major on the device, R right-handed in the cube / latitude-longitude frame above (+y towards tv = 0),
 * the rotated environment env_R(d) = env(R^T d); cubemap is [n_rot,6,res_y,res_x,C].  Per texel the expressions above with
 * the normalised direction replaced by R^T dir (three multiply-adds per component, in column order); a matrix that is
 * exactly the identity skips the product, so its slice equals gigs_latlong_to_cubemap bit for bit.  The result is the
 * rotated BASE: pre-filter it like any other light (the reference's pre-filters are not rotation-covariant, DESIGN.md
 * "Turntables").  1 <= n_rot <= 1024, else GIGS_ERR_INVALID. */
int gigs_latlong_to_cubemap_rot(int res_y, int res_x, int lat_h, int lat_w, int channels, const float* latlong, int n_rot,
                                const float* rotations, float* cubemap, void* stream);
int gigs_cube_texture_bwd(int res, int n, const float* dirs, const float* g_out, float* d_cubemap, int planar,
                          void* stream);
/* The lookup's backward as a gather, for a direction set that does not change between calls (the envmap TV's panorama grid).
 * gigs_cube_taps exports the four taps of every direction (idx [n,4] texel index or -1, w [n,4]); the caller sorts the valid
 * ones by texel into a CSR list -- offsets [6 res^2 + 1], ent_sample / ent_w in sample order within a texel -- and
 * gigs_cube_texture_bwd_gather writes EVERY texel of d_cubemap (no zero-fill needed) as the sum of its entries: one lane per
 * texel, one wave for each of the n_heavy texels (heavy_ids) that hold more than `heavy` entries.  No atomics: reproducible. */
int gigs_cube_taps(int res, int n, const float* dirs, int* idx, float* w, void* stream);
int gigs_cube_texture_bwd_gather(int res, int n, int planar, const int* offsets, const int* ent_sample, const float* ent_w,
                                 int heavy, int n_heavy, const int* heavy_ids, const float* g_out, float* d_cubemap,
                                 void* stream);

/* Training-loop glue (gigs-hip extension): the image losses of train.py and the Adam step, one
 * pass each.  Planes are [C,H,W] fp32; `scratch` holds at least gigs_loss_scratch_floats(C,H,W) floats (per-workgroup
 * partial sums, added in a fixed order -> reproducible losses); g_loss is a device scalar (NULL = 1).
 * gigs_l1_ssim_fwd = train.py:318-320 with utils/loss_utils.py:19-20, 55-98:
 *   out3 = {(1-lambda)*mean|image-gt| + lambda*(1-mean(ssim_map)), mean|image-gt|, mean(ssim_map)}; window 11,
 *   sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2.  d_mu1/d_e11/d_e12 [C,H,W] (all or none) receive the
 *   per-pixel derivatives of ssim_map that gigs_l1_ssim_bwd spreads back through the window into g_image.
 * gigs_tv_loss_fwd/bwd = get_tv_loss(gt, prediction, pad=1, step) (train.py:83-113) or, with mask_f [H,W] != NULL,
 *   get_masked_tv_loss without erosion (train.py:116-142); gt is [3,H,W] (NULL = no guide image, all pair weights 1:
 *   the plain TV of train.py:419-421), prediction [C,H,W]; gradient to prediction.
 * gigs_masked_l1_fwd/bwd = F.l1_loss(a[:, mask], b[:, mask]) (train.py:327), mask u8 [H,W];
 *   loss_count = {loss, number of mask pixels}; g_a / g_b may each be NULL (g_b = -g_a).
 * gigs_adam_step = torch.optim.Adam(eps=..., betas=...) without weight decay / amsgrad, as the reference configures it
 *   (scene/gaussian_model.py:325-346), for all parameter groups in one launch per 16 groups; `step` is the 1-based
 *   update count of the group's state, `lr` its current learning rate; zero_grad != 0 also clears the gradients.
 *   grad == NULL: the group's gradient is an exact zero that was not materialised -- the update runs with g = 0 (the
 *   moments decay, the parameter follows its momentum), which is NOT torch's "grad is None: skip the parameter". */
typedef struct gigs_adam_group {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long n;
  double lr;
  int step;
} gigs_adam_group;
size_t gigs_loss_scratch_floats(int channels, int height, int width);
int gigs_l1_ssim_fwd(int channels, int height, int width, const float* image, const float* gt, float lambda_dssim,
                     float* d_mu1, float* d_e11, float* d_e12, float* scratch, float* out3, void* stream);
int gigs_l1_ssim_bwd(int channels, int height, int width, const float* image, const float* gt, float lambda_dssim,
                     const float* d_mu1, const float* d_e11, const float* d_e12, const float* g_loss, float* g_image,
                     void* stream);
/* Per-view evaluation metrics (render.py's NVS loop and eval_brdf, normal_eval.py), reduced in double in a fixed order:
 * the same record bit for bit on every run.  `scratch` holds gigs_image_metrics_scratch_bytes(C,H,W) bytes (enough for
 * both entries with C = 3).  slot == NULL: the record goes to out; otherwise to out + stride * (*slot), and *slot (a
 * device int) is incremented, so a replayed graph fills successive records without a host synchronisation.
 * gigs_image_metrics: pred / gt [C,H,W]; record (stride C + 4) = {mse_c of utils/image_utils.py:31-33 per channel,
 *   mean over c of 20 log10(1 / sqrt(mse_c)) (psnr(a, b).mean()), mean(ssim_map) (utils/loss_utils.py:55-98: the
 *   ssim_map of gigs_l1_ssim_fwd), ((pred - gt) ** 2)[:, mask].mean() (render.py:601-603; mask u8 [H,W], NULL or empty:
 *   NaN), the number of masked elements}.
 * gigs_normal_angular_error: normal_eval.py:11-18 on the images render.py writes and normal_eval.py reads: pred [3,H,W]
 *   is the float plane render.py saves ((normal + 1) / 2), rounded to 8 bits as torchvision's save_image rounds it;
 *   gt [H,W,gt_channels] u8 is the ground-truth PNG (alpha = last channel, normal_eval.py:40).  Record (stride 2) =
 *   {sum of arccos(clip(<gt, pred>, -1, 1)) * 180 / pi, pixel count}. */
size_t gigs_image_metrics_scratch_bytes(int channels, int height, int width);
int gigs_image_metrics(int channels, int height, int width, const float* pred, const float* gt, const uint8_t* mask,
                       void* scratch, int* slot, double* out, void* stream);
int gigs_normal_angular_error(int height, int width, const float* pred, const uint8_t* gt, int gt_channels,
                              void* scratch, int* slot, double* out, void* stream);
/* LPIPS with the VGG16 backbone (lpips 0.1: net="vgg", lpips=True, spatial=False, eval mode), forward only, f32
 * arithmetic (the convolutions on f32-input MFMA), the value reduced in double in a fixed order: the same bits on every
 * call, for an image alone or inside a batch, and for (a, b) and (b, a).
 * gigs_lpips_vgg_pack: the 13 conv weights [Cout,Cin,3,3] and biases [Cout] of torchvision's vgg16().features (indices
 *   0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28; host array of device pointers) and the 5 lin weights [C] (lpips'
 *   lin{k}.model.1.weight) -> `packed` (gigs_lpips_vgg_weight_floats() floats), the layout gigs_lpips_vgg reads.
 * gigs_lpips_vgg: in0 / in1 [n,3,H,W] planar fp32 (normalize != 0: 2x - 1 first); H, W >= 16, else GIGS_ERR_INVALID.
 *   `scratch` holds gigs_lpips_vgg_scratch_bytes(n,H,W) bytes (0 for an invalid size).  Record of image i (stride 6) =
 *   {lpips, mean d of tap 0 .. 4} at out + 6 (*slot + i) and *slot += n (slot == NULL: out + 6 i), as
 *   gigs_image_metrics.  taps: NULL, or 10 device pointers that receive the raw taps (after the ReLU of conv1_2, conv2_2,
 *   conv3_3, conv4_3, conv5_3; [n,C,H_l,W_l]) of in0 (taps[0..4]) and in1 (taps[5..9]).  No host synchronisation and no
 *   allocation: safe to capture in a graph. */
size_t gigs_lpips_vgg_weight_floats(void);
int gigs_lpips_vgg_pack(const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, float* packed,
                        void* stream);
size_t gigs_lpips_vgg_scratch_bytes(int n, int height, int width);
int gigs_lpips_vgg(int n, int height, int width, const float* in0, const float* in1, int normalize, const float* packed,
                   void* scratch, int* slot, double* out, float* const* taps, void* stream);
/* Writing images (gigs-hip extension; the device half of image_writer.py): float planes -> 8-bit RGB sheets -> the
 * scanline stream of a PNG, i.e. everything of an encoder but the deflate.  `desc` is a DEVICE table of n descriptors
 * (0 <= n <= GIGS_MAX_IMAGES); all images go through one launch.  No host synchronisation and no allocation: safe to
 * capture in a graph, and the table may be rewritten between replays.  A descriptor with a NULL pointer, a size <= 0 or
 * channels outside {1, 3} is skipped; the caller is responsible for the bounds the descriptors imply.
 * gigs_pack_images: src [channels,H,W] fp32 -> dst[y * dst_stride + 3 * (dst_x + x) + c] (bytes; channels == 1 is
 *   replicated to three, as torchvision's make_grid does for save_image).  v = trunc(clamp(x * 255 + bias, 0, 255)) with
 *   the product and the sum rounded separately, which is bit for bit torch's x.mul(255).add_(bias).clamp_(0, 255)
 *   .to(torch.uint8): bias = 0.5 is torchvision.utils.save_image, bias = 0 is ToPILImage's mul(255).byte() (the latter
 *   stated from memory of torchvision's source, which was not at hand to check).  NaN -> 0 (torch leaves the conversion
 *   of NaN to uint8 undefined); +inf -> 255, -inf -> 0.  lohi != NULL: two device floats {lo, hi}, and
 *   x = (x - lo) / (hi - lo) (correctly rounded division) comes first: render.py:376's depth image.
 * gigs_plane_minmax: {min, max} of count floats -> out2 (device), through `scratch` (GIGS_MINMAX_SCRATCH_FLOATS floats)
 *   in a fixed order without float atomics.  NaNs are ignored (torch's min() / max() would propagate them).
 * gigs_png_filter: sheet [H, stride bytes] with 3 * width bytes used per row -> out, H * (1 + 3 * width) bytes: per row
 *   the filter type, then the filtered row (PNG specification, section 9: None, Sub, Up, Average, Paeth with bpp = 3;
 *   the row above row 0 and the pixel left of pixel 0 are zero).  Each row takes the filter with the smallest sum of
 *   |residual as int8| (libpng's heuristic); ties go to the lowest filter type. */
#define GIGS_MAX_IMAGES 4096
#define GIGS_MINMAX_SCRATCH_FLOATS 512
typedef struct gigs_pack_desc {
  const float* src;
  uint8_t* dst;
  const float* lohi;
  int channels, height, width;
  int dst_x;      /* pixels */
  int dst_stride; /* bytes per sheet row */
  float bias;
} gigs_pack_desc;
typedef struct gigs_filter_desc {
  const uint8_t* sheet;
  uint8_t* out;
  int height, width;
  int stride; /* bytes per sheet row */
  int reserved;
} gigs_filter_desc;
int gigs_pack_images(int n, const gigs_pack_desc* desc, void* stream);
int gigs_plane_minmax(long long count, const float* src, float* scratch, float* out2, void* stream);
int gigs_png_filter(int n, const gigs_filter_desc* desc, void* stream);
/* Meshes (gigs-hip extension; the device half of mesh.py): TSDF fusion of rendered planes into a volume, and naive
 * surface nets on the volume.  The volume: samples s(i,j,k) = lo + (i,j,k) voxel, i < dims[0] (fastest), j < dims[1],
 * k < dims[2], each axis 1..GIGS_TSDF_MAX_AXIS and fewer than 2^31 samples G; device arrays tsdf [G] (initially 1),
 * weight [G] (0), attr_weight [G] (0) and attr [8][G] (0; planar: world normal xyz, albedo rgb, roughness, metallic), all
 * fp32.  The two structures are HOST memory; the calls neither synchronise nor allocate.
 * gigs_tsdf_integrate: applies n_views (0..GIGS_TSDF_MAX_VIEWS) views in order, one thread per sample, no atomics: the
 *   result is deterministic, and n views in one call equal n calls of one view bit for bit.  Per sample and view, every
 *   product and sum rounded on its own and IEEE division:
 *     p = xform_point_4x3(s, viewmatrix) (the rasterizer's layout: m[0], m[4], m[8], m[12] make x);  p.z <= 0.2: skip
 *     u = p.x / p.z * fx + (W - 1) / 2, v = p.y / p.z * fy + (H - 1) / 2 with fx = W / (2 tanfovx), fy = H / (2 tanfovy):
 *       the pixel convention of the rasterizer's ndc2pix;  pixel (floor(u + 0.5), floor(v + 0.5)), outside the image: skip
 *     O = opacity, D = depth at that pixel.  O < opacity_min is background: with carve the sample is free space (d = 1,
 *       no attributes), without carve it is skipped.  Otherwise sdf = D - p.z; not sdf >= -trunc: skip;
 *       d = min(1, sdf / trunc)
 *     tsdf = (tsdf * weight + d) / (weight + 1), weight += 1; if not background and sdf <= trunc, each attribute the same
 *       way with attr_weight, then attr_weight += 1
 *   planes: opacity, depth, roughness, metallic [H,W]; normal, albedo [3,H,W].
 * gigs_mesh_count: cell_flags [(dims[0]-1)(dims[1]-1)(dims[2]-1)] (x fastest) = 1 for an active cell (all eight samples
 *   have weight >= min_weight and the signs of tsdf differ; tsdf < 0 is inside), else 0; sample_quads [G] = how many of a
 *   sample's +x, +y, +z edges get a quad (ends differ in sign, the four cells around the edge exist and are valid).
 *   Needs every axis >= 2.
 * gigs_mesh_write: cell_offsets / quad_offsets = the exclusive prefix sums of those arrays.  One vertex per active cell,
 *   vertex cell_offsets[cell]: position lo + (cell index + mean offset of the zero crossings f0 / (f0 - f1) on the cell's
 *   edges whose ends differ in sign, the 12 edges in a fixed order) voxel; attributes = the sum over the same crossings'
 *   endpoints of (interpolation weight) x (sample attribute) over the sum of the weights, where an endpoint with
 *   attr_weight == 0 has weight 0 (no endpoint left: 0); the normal is normalised last, a zero normal stays zero.  Two
 *   triangles (a fixed diagonal) per quad at faces[6 (quad_offsets[sample] + quads of lower axes)], counter-clockwise
 *   as seen from the positive end.  vertices, normals, albedo [vertex_capacity,3], roughness, metallic
 *   [vertex_capacity], faces [face_capacity,3] int32: an index outside a capacity sets *overflow (device int, cleared
 *   by the caller) to 1 and stores nothing. */
#define GIGS_TSDF_MAX_VIEWS 8
#define GIGS_TSDF_MAX_AXIS 1024
typedef struct gigs_tsdf_grid {
  float lo[3];
  float voxel;
  int dims[3];
  float trunc, opacity_min;
  int carve;
  float *tsdf, *weight, *attr_weight, *attr;
} gigs_tsdf_grid;
typedef struct gigs_tsdf_view {
  float viewmatrix[16];
  float tanfovx, tanfovy;
  int width, height;
  const float *opacity, *depth, *normal, *albedo, *roughness, *metallic;
} gigs_tsdf_view;
int gigs_tsdf_integrate(const gigs_tsdf_grid* grid, int n_views, const gigs_tsdf_view* views, void* stream);
int gigs_mesh_count(const gigs_tsdf_grid* grid, float min_weight, int* cell_flags, int* sample_quads, void* stream);
int gigs_mesh_write(const gigs_tsdf_grid* grid, float min_weight, const int* cell_offsets, const int* quad_offsets,
                    int vertex_capacity, int face_capacity, float* vertices, float* normals, float* albedo, float* roughness,
                    float* metallic, int* faces, int* overflow, void* stream);
/* Cleaning meshes (gigs-hip extension; the device half of mesh.components / mesh.clean): the connected components of a
 * triangle mesh, a keep flag per component, and the compaction of what is kept.  The mesh: V vertices, faces [F,3] int32,
 * and mesh.py's per-vertex arrays.  All arrays are DEVICE memory; the calls neither synchronise nor allocate.  Every
 * quantity below is an integer that does not depend on the order of execution (tests/mesh_clean_ref.py restates them).
 *   Valid face: all three indices lie in [0, V).  An invalid face is never dereferenced and belongs to no component:
 *     face_label = -1, never kept, counted in *invalid_faces.
 *   Connectivity: two vertices are connected if a chain of valid faces joins them, consecutive faces sharing AT LEAST ONE
 *     VERTEX.  This is vertex connectivity, not edge connectivity: two shells that touch in a single vertex are one
 *     component (the cheaper rule, and the conservative one for a filter: it never splits what an edge rule joins).  A
 *     degenerate face (a, a, b) is valid and connects a and b.
 *   label[v] = the smallest vertex index of v's component; a vertex no valid face references is a component of its own
 *     with zero faces (label[v] = v).  face_label[f] = label[faces[f,0]].  count[r] = the number of valid faces with
 *     face_label == r.  The components are the roots (label[v] == v) with count >= 1, in ascending root order.
 *   Keep rule (mesh.keep_threshold; the 2DGS post-processing threshold with keep_largest = K, min_faces = M): c_K = the K-th
 *     largest count among the components, 0 when K <= 0, the smallest count when K >= their number; a component is kept
 *     iff count >= max(M, c_K, 1), so components tied with the K-th are all kept.
 *   Compaction: a vertex is kept iff a kept face references it, its new index is the number of kept vertices with a
 *     smaller index; kept faces stay in their order with remapped indices and unchanged winding; positions and the five
 *     attribute arrays are copied bit for bit.
 * gigs_mesh_cc_hook, one thread per face: `parent` [V] int32 with 0 <= parent[x] <= x, set to parent[x] = x by the CALLER
 *   before the first call.  The three roots of a valid face by walking parent (a walk down a strictly decreasing chain:
 *   it ends by itself, and a value outside [0, x) ends it too), m = their minimum, atomicMin(parent[r], m) for each root
 *   r > m.  *changed (device int, cleared inside the call) becomes 1 if some face saw different roots.
 * gigs_mesh_cc_flatten, one thread per vertex: parent[v] = root(v).
 *   The caller alternates hook and flatten until a hook leaves *changed == 0; parent is then label.  That confirming pass
 *   stored nothing, so every face was seen under one root of a static forest; a link that a stale read overwrote in an
 *   earlier pass is re-made by the pass after it (gi-gs_amd/csrc/mesh_clean.hip has the argument).  No call waits on
 *   another thread: there is no retry, spin or ticket loop.
 * gigs_mesh_cc_count, one thread per face, parent = label: face_label [F]; count [V] and *invalid_faces (cleared inside
 *   the call) by integer atomics, one per wave for the lanes that share the label of the wave's first valid lane.
 * gigs_mesh_mark, one thread per face: face_keep [F] int32 = 1 for a valid face with root_keep[face_label] != 0
 *   (root_keep [V] uint8), else 0; vertex_keep [V] int32 (cleared inside the call) = 1 for the vertices of those faces.
 * gigs_mesh_compact: vertex_offsets / face_offsets = the exclusive prefix sums of vertex_keep / face_keep.  Kept vertex v
 *   goes to row vertex_offsets[v] of out_vertices, out_normals, out_albedo [vertex_capacity,3], out_roughness,
 *   out_metallic [vertex_capacity]; kept face f to row face_offsets[f] of out_faces [face_capacity,3] with its indices
 *   replaced by vertex_offsets.  A row outside a capacity, a new index outside [0, vertex_capacity), or a kept face with
 *   an index outside [0, V) or on a vertex that is not kept sets *overflow (device int, cleared by the caller) to 1 and
 *   stores nothing: gigs_mesh_write's guard. */
int gigs_mesh_cc_hook(int n_vertices, int n_faces, const int* faces, int* parent, int* changed, void* stream);
int gigs_mesh_cc_flatten(int n_vertices, int* parent, void* stream);
int gigs_mesh_cc_count(int n_vertices, int n_faces, const int* faces, const int* parent, int* face_label, int* count,
                       int* invalid_faces, void* stream);
int gigs_mesh_mark(int n_vertices, int n_faces, const int* faces, const int* face_label, const uint8_t* root_keep,
                   int* face_keep, int* vertex_keep, void* stream);
int gigs_mesh_compact(int n_vertices, int n_faces, const float* vertices, const float* normals, const float* albedo,
                      const float* roughness, const float* metallic, const int* faces, const int* vertex_keep,
                      const int* vertex_offsets, const int* face_keep, const int* face_offsets, int vertex_capacity,
                      int face_capacity, float* out_vertices, float* out_normals, float* out_albedo, float* out_roughness,
                      float* out_metallic, int* out_faces, int* overflow, void* stream);
/* Simplifying meshes (gigs-hip extension; the device half of mesh.cluster_map / mesh.simplify): vertex clustering on a
 * uniform grid of cells (Rossignac-Borrel) with one representative vertex per cell placed by its faces' plane quadrics
 * (Lindstrom).  simplify(mesh, cell, origin = NULL, reg = 1e-3); cell > 0 in world units.  All arrays are DEVICE memory
 * except `origin` (three floats on the host, read during the call); the calls neither synchronise nor allocate; the sorts
 * and scans between them are the caller's.  No float atomics and no thread waits on another: the output bits do not
 * depend on the order of execution (tests/mesh_simplify_ref.py restates everything below in numpy).
 *   1 Cells.  origin defaults to the per-axis minimum over the finite vertices (float32).  inv = float32(1) / float32(cell).
 *     A vertex v has the cell c = floor((v - origin) * inv) per axis: one float32 subtraction, one float32 product (no
 *     contraction: __fsub_rn, __fmul_rn), floorf.  key = cx | cy << 21 | cz << 42 (int64).  A vertex with a non-finite
 *     coordinate, or with a cell coordinate outside [0, 2^21) (possible only under an explicit origin), is UNCLUSTERED:
 *     key = -1, cluster -1, it joins no cluster.  The host reads the extent of the finite vertices back once and refuses
 *     (ValueError) a mesh whose extent, measured from its own minimum, needs a cell coordinate >= 2^21 on some axis.
 *   2 Clusters.  The distinct keys >= 0 in ascending order are the clusters 0 .. C-1; the members of a cluster are taken in
 *     ascending vertex index (a stable sort of the keys gives both orders).  cluster_of [V] int32.
 *   3 Faces.  A face is VALID if its three indices lie in [0, V) and its three vertices are clustered.  A valid face whose
 *     three clusters are pairwise different SURVIVES as the triple of its clusters, rotated so that the smallest comes first
 *     (winding unchanged); every other face becomes (-1, -1, -1).  Among surviving faces with the same rotated triple only
 *     the one with the lowest face index stays, the others become (-1, -1, -1).  Faces on the same three clusters with
 *     OPPOSITE winding have different triples and both stay (the two sides of a collapsed thin part).
 *   4 Attributes of a cluster.  albedo, roughness, metallic: the float64 sum of the members' values in ascending vertex
 *     index, divided by the member count, rounded once to float32.  normal: the float64 member sum s divided by
 *     sqrt(s . s) component by component, or zero if that length is zero.
 *   5 Position of a cluster, in float64 and in coordinates local to the cell centre g = origin + (c + 1/2) cell: every
 *     valid face, surviving or not, contributes once to each distinct cluster among its three, in ascending face index,
 *     its area-weighted plane quadric: n = (p1 - p0) x (p2 - p0), u = n / |n|, w = |n| / 2, d = -(u . p0); A += w u u^T,
 *     b += w d u; faces with |n| = 0 add nothing.  m = the member mean (local), lam = reg (A00 + A11 + A22) / 3.  If
 *     lam > 0 is false (no area), x = m; else x solves (A + lam I) x = lam m - b (symmetric positive definite, condition
 *     <= 3 / reg + 1; by cofactors).  x is clamped per axis to [-cell / 2, cell / 2]; the position is float32(g + x).  The
 *     clamp is continuous: there is no accept-or-fall-back decision that two implementations could take differently.
 *   6 Compaction.  The C cluster vertices and the rewritten faces go through gigs_mesh_mark (every face label 0,
 *     root_keep[0] = 1) and gigs_mesh_compact: the (-1, -1, -1) rows and the clusters no kept face references go, order
 *     is kept.
 * gigs_mesh_cluster_keys, one thread per vertex: keys [V] int64 as in 1, inv_cell = inv.
 * gigs_mesh_cluster_faces, one thread per face: triples [F,3] int32 as in 3 before the removal of duplicates; pair_keys
 *   [3 F] int64: slot j of face f holds cluster << 32 | f if the face is valid and the cluster of its j-th vertex differs
 *   from those of the earlier slots, else 2^63 - 1, so the sorted array lists every cluster's faces in ascending face
 *   index and the sentinels last.  cluster_of entries outside [0, n_clusters) count as unclustered.  counts [2] (cleared
 *   inside the call; integer atomics): the invalid faces, and the valid faces with a repeated cluster.
 * gigs_mesh_face_dedupe, one thread per row of `order` [F] int64 (the faces sorted by triple, ties in ascending face
 *   index): out_faces [F,3] (set to -1 inside the call) receives the triple of every surviving face that differs from its
 *   predecessor's; *duplicates (cleared inside the call) counts the others.
 * gigs_mesh_cluster_solve, one thread per cluster: member_order [V] int64 = the vertices sorted by (key, index),
 *   member_start [C + 1] int64 = the first row of every cluster in it and the end of the last, pair_keys [3 F] SORTED,
 *   pair_start [C + 1] int64 = the first row of every cluster in it (the first key >= k << 32), cluster_keys [C] int64.
 *   Writes 4 and 5 into out_vertices, out_normals, out_albedo [C,3], out_roughness, out_metallic [C].
 * An order row, an offset, a pair key or a face index outside its range sets *overflow (device int, cleared by the
 *   caller) to 1 and the thread stores nothing: gigs_mesh_compact's convention. */
int gigs_mesh_cluster_keys(int n_vertices, const float* vertices, const float* origin, float inv_cell, long long* keys,
                           void* stream);
int gigs_mesh_cluster_faces(int n_vertices, int n_faces, int n_clusters, const int* faces, const int* cluster_of, int* triples,
                            long long* pair_keys, int* counts, void* stream);
int gigs_mesh_face_dedupe(int n_faces, const int* triples, const long long* order, int* out_faces, int* duplicates,
                          int* overflow, void* stream);
int gigs_mesh_cluster_solve(int n_vertices, int n_faces, int n_clusters, const float* vertices, const float* normals,
                            const float* albedo, const float* roughness, const float* metallic, const int* faces,
                            const long long* member_order, const long long* member_start, const long long* pair_keys,
                            const long long* pair_start, const long long* cluster_keys, const float* origin, float cell,
                            double reg, float* out_vertices, float* out_normals, float* out_albedo, float* out_roughness,
                            float* out_metallic, int* overflow, void* stream);
/* Comparing meshes (gigs-hip extension; the device half of mesh.sample_surface / mesh.closest_point / mesh.distance):
 * area-weighted samples of a surface and, for every query point, the exact closest triangle of a mesh through a uniform
 * grid of triangle lists.  All arrays are DEVICE memory except `lo` (three floats) and `dims` (three ints) on the host,
 * read during the call; the calls neither synchronise nor allocate; the sorts and scans between them are the caller's.  One
 * independent thread per face, sample or query, no float atomics, no thread waits on another: the output bits do not
 * depend on the order of execution (tests/mesh_distance_ref.py restates everything below in numpy).  All arithmetic below
 * is float64 on the float32 inputs, every product and sum rounded on its own; dot(a, b) = (a0 b0 + a1 b1) + a2 b2,
 * cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 *   1 Usable faces.  A face is USABLE if its three indices lie in [0, V), its nine coordinates are finite and |n| > 0 with
 *     n = cross(p1 - p0, p2 - p0), |n| = sqrt(dot(n, n)).  area = |n| / 2; an unusable face has area 0, gets no sample, is
 *     in no grid cell and is counted in *skipped.
 *   2 Random numbers.  mix(z): z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31 (the
 *     splitmix64 finaliser, uint64).  u(i, k) = (mix((seed 2^32 + i) 4 + k) >> 11) 2^-53, in [0, 1).
 *   3 Samples.  cum [F] = the inclusive cumulative sum of the areas, A = cum[F - 1] > 0.  Sample i of n: t = ((i + u(i, 0))
 *     / n) A; its face is the first f with cum[f] > t, and if there is none (t rounded up to A) the first f with
 *     cum[f] >= A: the last usable face.  (a, b) = (u(i, 1), u(i, 2)), replaced by (1 - a, 1 - b) if a + b > 1.
 *     point = float32((p0 + a (p1 - p0)) + b (p2 - p0)) per component; bary = (float32(a), float32(b)).
 *   4 Grid.  lo = the minimum corner of the usable faces (float32), cell > 0, dims = (Gx, Gy, Gz) each in [1, 256].  The
 *     cell coordinate of x on axis a is c(x) = clamp(floor((x - lo_a) / cell), 0, G_a - 1); the cell planes are
 *     plane_a(k) = lo_a + k cell; cell index = (z Gy + y) Gx + x.  A usable face is listed in every cell of the box
 *     [c(min corner), c(max corner)] per axis.  pair key = cell << 32 | face (int64); the caller sorts the keys, and
 *     cell_start [Gx Gy Gz + 1] int64 = the first row of every cell (the first key >= cell << 32), so every list ascends
 *     in face index.
 *   5 Point-triangle.  seg(p; a, b): ab = b - a, ap = p - a, t = dot(ap, ab), den = dot(ab, ab); t <= 0: dot(ap, ap);
 *     t >= den: dot(p - b, p - b); else q = ap - (t / den) ab, dot(q, q).  The three edges are each walked from the
 *     vertex with the lower INDEX, so two faces that share an edge get the same bits from it.  d^2 = the minimum of the
 *     three; if the edge functions dot(cross(b - a, p - a), n) over (p0,p1), (p1,p2), (p2,p0) are all >= 0, the plane
 *     term dot(p - p0, n)^2 / dot(n, n) enters the minimum too.  On the border between the cases the candidates coincide.
 *     distance = float32(sqrt(d^2)).  Among faces with equal d^2 the smallest face index wins.
 *   6 Search.  c0 = the clamped cell of the query.  Round r = 0, 1, .. visits the cells of the grid at Chebyshev distance
 *     r from c0.  After it, L(r) = the minimum, over the sides of the block [c0 - r, c0 + r] that have cells behind them
 *     (c0_a - r > 0: p_a - plane_a(c0_a - r); c0_a + r < G_a - 1: plane_a(c0_a + r + 1) - p_a), of max(0, that distance);
 *     L' = (L - 2^-45 M)(1 - 2^-40) with M = the largest |lo_a| or |plane_a(G_a)|.  The search ends when no side has cells
 *     behind it, when L' > 0 and best d^2 <= L'^2, or when L' > max_distance; at most max(G) rounds.
 *   7 Results.  A query with a non-finite coordinate: distance +inf, face -1, counts[1] += 1.  A query whose best d^2 exceeds
 *     max_distance^2 (max_distance = +inf for no limit), or that met no face: distance float32(max_distance), face -1,
 *     counts[0] += 1.
 * gigs_mesh_face_areas, one thread per face: areas [F] float64 and *skipped (cleared inside the call) as in 1.
 * gigs_mesh_sample_surface, one thread per sample (a binary search over cum_areas): points [n,3], face [n], bary [n,2] as
 *   in 3.  n_samples == 0 launches nothing; with samples asked of no face the call fails.
 * gigs_mesh_grid_count, one thread per face: counts [F] int32 = the cells of the face's box, 0 for areas[f] <= 0.
 * gigs_mesh_grid_pairs, one thread per face: offsets [F] int64 = the exclusive cumulative sum of counts; the face's keys go
 *   to pair_keys[offsets[f] ..].  A range outside [0, n_pairs] sets *overflow and stores nothing.
 * gigs_mesh_closest, one thread per row of `order` [N] int64 (the queries sorted by cell, or NULL for the identity): query
 *   order[i] gets distance and face as in 5 - 7; counts [2] (cleared inside the call; integer atomics) = far, invalid.
 * An order row, a cell_start entry, a pair key (its cell is not the cell visited, its face >= F) or a face index outside its
 *   range sets *overflow (device int, cleared by the caller) to 1 and the thread stores nothing: gigs_mesh_compact's
 *   convention. */
int gigs_mesh_face_areas(int n_vertices, int n_faces, const float* vertices, const int* faces, double* areas, int* skipped,
                         void* stream);
int gigs_mesh_sample_surface(int n_vertices, int n_faces, const float* vertices, const int* faces, const double* cum_areas,
                             int n_samples, unsigned long long seed, float* points, int* face, float* bary, int* overflow,
                             void* stream);
int gigs_mesh_grid_count(int n_vertices, int n_faces, const float* vertices, const int* faces, const double* areas,
                         const float* lo, double cell, const int* dims, int* counts, void* stream);
int gigs_mesh_grid_pairs(int n_vertices, int n_faces, const float* vertices, const int* faces, const double* areas,
                         const float* lo, double cell, const int* dims, const long long* offsets, long long n_pairs,
                         long long* pair_keys, int* overflow, void* stream);
int gigs_mesh_closest(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                      const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                      int n_points, const float* points, const long long* order, double max_distance, float* distance,
                      int* face, int* counts, int* overflow, void* stream);
/* Baking occlusion (gigs-hip extension; the device half of mesh.raycast / mesh.bake_occlusion): the nearest usable face a
 * ray hits, searched through the triangle grid of "Comparing meshes", and on top of it the ambient occlusion of every
 * vertex.  All arrays are DEVICE memory except `lo` and `dims` (host, read during the call); the calls neither synchronise
 * nor allocate; the sorts before them are the caller's.  One independent thread per ray, no float atomics, no thread waits
 * on another.  All arithmetic is float64 on the float32 inputs, + - * / only, every product and sum rounded on its own
 * (dot and cross as under "Comparing meshes"): there is no sqrt and no transcendental, so tests/mesh_raycast_ref.py
 * reproduces every bit in numpy.
 *   1 Usable faces and the grid: 1 and 4 of "Comparing meshes".  A face that is in no grid cell cannot be hit.
 *   2 Edge functions.  For the ray (o, d) and the face (i0, i1, i2) with corners p0, p1, p2 let a_k = p_k - o.  The edge
 *     between the vertices j and k has s = dot(d, cross(a_lo, a_hi)) with (lo, hi) = (j, k) if i_j < i_k, else (k, j): the
 *     ends are always taken in ascending vertex INDEX.  w = s if i_j < i_k, else -s.  w0 is that of the edge 1 -> 2 (the
 *     edge opposite vertex 0), w1 of 2 -> 0, w2 of 0 -> 1.  Two faces that share an edge and traverse it in opposite
 *     directions compute the same bits with opposite signs: no ray passes between them.
 *   3 Inside.  The ray is inside iff w0, w1, w2 are all >= 0 or all <= 0, and not all zero.  Faces are two-sided.
 *   4 Plane.  n = cross(p1 - p0, p2 - p0), dn = dot(d, n).  The face is a candidate only if
 *     dn dn > 2^-40 (dot(d, d) dot(n, n)): a ray within about 10^-6 rad of the face's plane misses it BY DEFINITION.
 *     t = dot(a_0, n) / dn, and 0 <= t <= t_max is required.
 *   5 Box.  With sigma = 2^-26 (M + max(|o_x|, |o_y|, |o_z|)), M = `scale` = the largest |coordinate| of a corner of a usable
 *     face (the caller's; a larger value keeps the traversal complete but is another definition), the
 *     hit point x_a = o_a + t d_a must satisfy  min_k p_k,a - sigma <= x_a <= max_k p_k,a + sigma  on every axis.  Under
 *     the guard of 4 the rounding of t moves x by less than 2^-30 (M + |o|), so a ray through the face never fails this
 *     test; it bounds how far outside its face an ACCEPTED hit can lie, which the inside test alone does not (an edge
 *     function of a tiny edge far from o has no useful relative accuracy), and that bound is what makes the traversal
 *     provably complete ("Baking occlusion").  A face that passes 3, 4 and 5 is ACCEPTED.
 *   6 Result.  The minimum of (t, face index) over ALL accepted usable faces, float64 t compared, ties to the smaller
 *     index: a function of ray, mesh, t_max and M alone.  t = float32(t), bary = (float32(w1 / W), float32(w2 / W)),
 *     W = (w0 + w1) + w2.  A miss: +inf, -1, (0, 0).  A ray with a non-finite component or d = 0: the same, and
 *     counts[1] += 1; counts[0] counts the hits.
 *   7 Traversal.  A = the axis of the largest |d_a| (the lowest on a tie), U = A + 1 mod 3, W = A + 2 mod 3.  Slabs
 *     k = c_A(o_A -+ 3 sigma) (-: d_A > 0, +: d_A < 0) onwards in the direction of travel, at most G_A of them:
 *       ta = ((plane_A(k) - 2 sigma) - o_A) / d_A, tb = ((plane_A(k + 1) + 2 sigma) - o_A) / d_A, tn = min, tf = max;
 *       tf < 0: next slab;  tn > t_max or best t < tn: stop;  tn = max(tn, 0), tf = min(tf, t_max);
 *       on U (and W alike): y_n = o_U + tn d_U, y_f = o_U + tf d_U, cells c_U(min(y_n, y_f) - 2 sigma) ..
 *       c_U(max(y_n, y_f) + 2 sigma); every face listed in a cell of that rectangle of slab k is tested.
 *     |d_U| <= |d_A| keeps the rectangle at 3 x 3 cells while 8 sigma < cell; a ray whose origin is so far away that
 *     sigma reaches the cell size widens it, up to the slab.  Every accepted face is listed in a visited cell.
 *   8 Bake.  directions [K, R, 3] float32 in the local frame (z >= 0), R a multiple of 64 in [64, 1024], K in [1, 64].
 *     Vertex v with position p and stored normal n (float32 -> float64, NOT renormalised): if p is not finite or
 *     dot(n, n) is not in [1 - 2^-10, 1 + 2^-10], occlusion = 1, hits = 0 and counts[1] += 1.  Else, the basis of Duff et
 *     al. 2017: s = copysign(1, n_z), a = -1 / (s + n_z), b = (n_x n_y) a, T = (1 + ((s n_x) n_x) a, s b, (-s) n_x),
 *     B = (b, s + (n_y n_y) a, -n_y); rotation k = mix((seed 2^32 + v) mod 2^64) mod K; ray j of R: origin o_c = p_c +
 *     bias n_c, direction d_c = (x T_c + y B_c) + z n_c with (x, y, z) = directions[k, j], as doubles; hits = the rays with
 *     an accepted face at 0 <= t <= max_distance; occlusion = float32((R - hits) / R), 1 = open; counts[0] += hits.
 * gigs_mesh_raycast, one thread per row of `order` [N] int64 (the rays sorted by the cell they enter the grid in, or NULL):
 *   ray order[i] gets t [N], face [N], bary [N,2] as in 6; counts [2] int32 (cleared inside the call) = hits, invalid.
 *   n_rays == 0 launches nothing.
 * gigs_mesh_bake_occlusion, one one-wave block per row of `order` [V] int64 (the vertices sorted by cell, or NULL): the
 *   wave walks the vertex's R / 64 chunks of 64 directions, one per lane, and stores occlusion [V] float32 and hits [V]
 *   int32 itself; counts [2] uint64 (cleared inside the call) = hits in all, vertices without a normal.
 * An order row, a cell_start entry, a pair key or a face index outside its range sets *overflow (cleared by the caller) and
 *   the thread (the wave, in the bake) stores nothing. */
int gigs_mesh_raycast(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                      const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs, double scale,
                      int n_rays, const float* origins, const float* directions, const long long* order, double t_max, float* t,
                      int* face, float* bary, int* counts, int* overflow, void* stream);
int gigs_mesh_bake_occlusion(int n_vertices, int n_faces, const float* vertices, const float* normals, const int* faces,
                             const float* lo, double cell, const int* dims, const long long* cell_start,
                             const long long* pair_keys, long long n_pairs, double scale, const long long* order,
                             const float* directions, int n_rays, int n_rotations, unsigned long long seed, double max_distance, double bias,
                             float* occlusion, int* hits, unsigned long long* counts, int* overflow, void* stream);
/* Baking light (gigs-hip extension; the device half of mesh.trace_hemispheres / mesh.gather_light / mesh.bake_light): the
 * light every vertex receives from an environment cube, shadowed by the mesh and with any number of diffuse bounces.  The
 * hemisphere of every vertex is traced ONCE and every ray's hit is RECORDED (gigs_mesh_trace_hemisphere); every pass, and
 * every other environment, is one gather over the records (gigs_mesh_gather_light).  All arrays are DEVICE memory except
 * `lo` and `dims`; the calls neither synchronise nor allocate.  The conventions are those of "Baking occlusion": float64 on
 * the float32 inputs, + - * / only, every product and sum rounded on its own, no sqrt and no transcendental, no float
 * atomics: tests/mesh_light_ref.py reproduces every bit in numpy.
 *   1 Rays.  Those of "Baking occlusion", 8, by the same code: the table [K, R, 3], the rotation k, the basis (T, B, n), the
 *     origin o = p + bias n, the direction d_i = (x T + y B) + z n of row (k, i), and the no_normal rule.  Vertex v casts
 *     the rays i = 0 .. R - 1 of ITS rotation in every call: a gather rebuilds d_i from the table.
 *   2 Records.  Ray i of vertex v is traversed as in 2 to 7 there with t_max = max_distance (+inf: no limit; a face beyond
 *     it is not accepted, the ray then misses).  hit_face [V, R] int32: a miss is -1.  For the winning face f let
 *     n_g = cross(p1 - p0, p2 - p0) of its corners and s = dot(d, n_g) (not 0 under the guard of 4): s < 0 is a FRONT hit,
 *     recorded as f; otherwise a BACK hit, recorded as -2 - f: the ray reached the inside of a shell, which carries no
 *     light.  hit_bary [V, R, 2] float32 = (float32(w1 / W), float32(w2 / W)) as gigs_mesh_raycast writes them; (0, 0) on
 *     a miss.  A no_normal vertex gets -1 and (0, 0) in all its records and counts[3] += 1; its rays are in no other
 *     counter.  counts [4] uint64 (cleared inside the call) = misses, front hits, back hits, no_normal vertices.
 *   3 Sky.  sky [6, n, n, 3] float32, the cube of the lights (cube.h, cube_face_uv; the cube's axes are the world's).  For a
 *     direction (x, y, z): if |z| > max(|x|, |y|): face 4, c = z, (a, b) = (x, y); else if |y| > |x|: face 2, c = y,
 *     (a, b) = (x, z); else face 0, c = x, (a, b) = (z, y); face += 1 if c < 0.  m = 0.5 / |c|; m0 = -m on the faces 0 and
 *     5, else m; m1 = m on face 2, else -m; u = min(max(a m0 + 0.5, 0), 1), v = min(max(b m1 + 0.5, 0), 1); texel
 *     ix = min(n - 1, floor(u n)), iy = min(n - 1, floor(v n)) (a NaN goes to texel 0): sky[face, iy, ix], the nearest
 *     texel, unfiltered.
 *   4 Contribution c_i of ray i, three float64 values.  Miss: the sky texel of d_i.  Front hit of face f = (i0, i1, i2) with
 *     `previous` [V, 3] float32 given: b1, b2 = the record's float32 weights as doubles, b0 = max(0, (1 - b1) - b2),
 *     c = (b0 Q[i0] + b1 Q[i1]) + b2 Q[i2], Q = previous as doubles.  A back hit, or any hit with previous == NULL: 0.
 *   5 Sum.  Lane l of the wave adds c_i for i = l, l + 64, l + 128, .. in that order, starting from 0.0; then
 *     S_l <- S_l + S_(l xor s) for s = 32, 16, 8, 4, 2, 1, all lanes at once: IEEE addition is commutative, so all lanes hold
 *     the same bits.  irradiance[v] = float32(S / R); radiosity[v] = float32(double(reflectance[v]) double(irradiance[v])),
 *     per channel.  A no_normal vertex (rule 1, from `vertices` and `normals`) gets 0 in both.
 *   6 Passes.  I(0) = gather with previous = NULL: the shadowed sky.  I(b) = gather with previous = the radiosity of pass
 *     b - 1: a Jacobi iteration over the same rays.  The irradiance is the cosine-weighted MEAN of the incoming radiance,
 *     the normalisation of the shade's diffuse cube: a constant sky c on an open vertex gives c.
 * gigs_mesh_trace_hemisphere, one one-wave block per row of `order` [V] int64 (the vertices sorted by cell, or NULL): the
 *   wave walks the R / 64 chunks, one direction per lane, and stores 64 records side by side per chunk.
 * gigs_mesh_gather_light, one one-wave block per vertex; sky_res = n in [1, 4096].  n_vertices == 0 launches nothing.
 * An order row, a cell_start entry, a pair key, a face index or a record (f or -2 - f not in [0, F)) outside its range sets
 *   *overflow (cleared by the caller) and the wave stores nothing from then on. */
int gigs_mesh_trace_hemisphere(int n_vertices, int n_faces, const float* vertices, const float* normals, const int* faces,
                               const float* lo, double cell, const int* dims, const long long* cell_start,
                               const long long* pair_keys, long long n_pairs, double scale, const long long* order,
                               const float* directions, int n_rays, int n_rotations, unsigned long long seed, double max_distance,
                               double bias, int* hit_face, float* hit_bary, unsigned long long* counts, int* overflow, void* stream);
int gigs_mesh_gather_light(int n_vertices, int n_faces, const float* vertices, const float* normals, const int* faces,
                           const float* directions, int n_rays, int n_rotations, unsigned long long seed, const int* hit_face,
                           const float* hit_bary, int sky_res, const float* sky, const float* reflectance, const float* previous,
                           float* irradiance, float* radiosity, int* overflow, void* stream);
/* Ray-traced light per point (gigs-hip extension; the device half of mesh.gather_points / mesh.final_gather): "Baking
 * occlusion" and "Baking light" for ANY set of surface points with normals -- in practice the covered pixels of a G-buffer --
 * in one kernel, a lightmap final gather: the open share of the hemisphere, the irradiance under the environment cube
 * shadowed by the mesh, and the diffuse light bounced from the mesh's baked radiosity.  The conventions are those of the two
 * sections: DEVICE arrays except `lo` and `dims`, no synchronisation, no allocation, float64 on the float32 inputs, + - * /
 * only, no sqrt, no float atomics: tests/mesh_gather_ref.py reproduces every bit in numpy.
 *   1 Points.  points [N, 3], normals [N, 3] float32; mask [N] uint8 or NULL.  Point q with mask[q] == 0 is MASKED
 *     (counts[4] += 1); otherwise a point that fails the no_normal rule of "Baking occlusion", 8 (position not finite,
 *     dot(n, n) not in [1 - 2^-10, 1 + 2^-10]) counts as no_normal (counts[3] += 1).  Either way hits = 0, occlusion = 1 and
 *     both light outputs are 0; its rays are in no other counter.
 *   2 Rays.  Those of "Baking occlusion", 8, by the same code with the point in the vertex's place: the rotation
 *     k = mix((seed 2^32 + q) mod 2^64) mod K, the basis of the point's normal, the origin o = p + bias n, the direction of
 *     row (k, i) of the table [K, R, 3].
 *   3 Classification.  Ray i is traversed as in 2 to 7 there with t_max = max_distance (+inf: no limit) and classified as in
 *     "Baking light", 2: a miss, a FRONT hit (dot(d, n_g) < 0) or a BACK hit.  counts[0..2] = misses, front hits, back hits.
 *   4 Occlusion.  hits[q] = the rays whose nearest accepted face has t <= ao_distance (float64 t);
 *     occlusion[q] = float32(double(R - hits) / double(R)), 1 = open.
 *   5 Occlusion only.  With sky == NULL the rays are traversed with t_max = min(ao_distance, max_distance) (ao_distance, if
 *     max_distance is not the smaller), and irradiance and indirect are not touched (pass NULL).  hits is the same: whether a
 *     face is accepted at t does not depend on t_max >= t, so a ray has an accepted face within ao_distance exactly when
 *     its NEAREST accepted face lies there.  The counters 0..2 then classify within that distance.
 *   6 Light.  The contribution c_i of "Baking light", 4: a miss brings the sky texel of d_i (3 there); a front hit of face
 *     (i0, i1, i2) brings (b0 Q[i0] + b1 Q[i1]) + b2 Q[i2], Q = radiosity [V, 3] float32 as doubles (0 if radiosity ==
 *     NULL), b1 = double(float32(w1 / W)), b2 = double(float32(w2 / W)) -- the float32 rounding the records have --
 *     b0 = max(0, (1 - b1) - b2); a back hit brings 0.
 *   7 Sums.  Lane l adds c_i for i = l, l + 64, .. in that order from 0.0 into S, and the front hits' c_i alone, in the same
 *     order, into S_ind; both go through the butterfly of "Baking light", 5.  irradiance[q] = float32(S / R),
 *     indirect[q] = float32(S_ind / R), per channel.  With the radiosity of pass b - 1 of gigs_mesh_gather_light and points
 *     = the vertices this is I(b) of "Baking light", 6, bit for bit.
 * gigs_mesh_gather_points, one one-wave block per row of `order` [N] int64 (the points sorted by cell, or NULL): the wave
 *   walks the R / 64 chunks, one direction per lane, and stores hits [N] int32, occlusion [N] float32, irradiance [N, 3] and
 *   indirect [N, 3] float32 itself; counts [5] uint64 (cleared inside the call) = misses, front hits, back hits, no_normal
 *   points, masked points.  sky_res = n in [1, 4096] when sky is given.  n_points == 0 launches nothing.
 * An order row, a cell_start entry, a pair key or a face index outside its range sets *overflow (cleared by the caller) and
 *   the wave stores nothing. */
int gigs_mesh_gather_points(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                            const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                            double scale, int n_points, const float* points, const float* normals, const unsigned char* mask,
                            const long long* order, const float* directions, int n_rays, int n_rotations, unsigned long long seed,
                            double ao_distance, double max_distance, double bias, int sky_res, const float* sky,
                            const float* radiosity, int* hits, float* occlusion, float* irradiance, float* indirect,
                            unsigned long long* counts, int* overflow, void* stream);
/* Ray-traced reflections per point (gigs-hip extension; the device half of mesh.reflect_points and
 * mesh_render.compose_reflections): the SPECULAR counterpart of the section above.  For the points of "Ray-traced light per
 * point", each with a view direction and a roughness, a GGX lobe of rays about the mirror direction is traced against the
 * mesh: the radiance the lobe brings (the first sum of the split-sum approximation, Karis 2013: the n.l-weighted mean over
 * half vectors drawn from the GGX distribution, here about the TRUE view direction and not under n = v = r), its share from
 * the mesh, and the open share of the lobe.  The conventions are that section's: DEVICE arrays except `lo` and `dims`, no
 * synchronisation, no allocation, float64 on the float32 inputs, + - * / only, no sqrt, no float atomics:
 * tests/mesh_reflect_ref.py reproduces every bit in numpy.
 *   1 Table.  directions [L, K, R, 3] float32: GGX-distributed HALF vectors in the tangent frame (z the normal), L = n_levels
 *     in [1, 64] roughness levels of K rotations of R rows (mesh.ggx_directions computes it on the host).
 *   2 Points.  points, normals, views [N, 3], roughness [N] float32; mask [N] uint8 or NULL.  Point q with mask[q] == 0 is
 *     MASKED (counts[6] += 1); otherwise a point that fails the no_normal rule of "Baking occlusion", 8 counts as no_normal
 *     (counts[4] += 1); otherwise, with v = views[q] (pointing from the surface TOWARDS the eye), a point whose v is not
 *     finite or has dot(v, v) outside [1 - 2^-10, 1 + 2^-10] counts as no_view (counts[5] += 1).  Such a point gets
 *     specular = reflected = 0, visibility = 1, valid = blocked = 0; its rays are in no other counter.
 *   3 Frame.  "Baking occlusion", 8, by the same code: the rotation k = mix((seed 2^32 + q) mod 2^64) mod K, the basis (T, B)
 *     of the point's normal n, the origin o = p + bias n.  The level is lev = min(L - 1, floor(roughness[q] L)), 0 for a NaN
 *     or a negative product; lane i of chunk j reads row (lev, k, 64 j + i) = (x, y, z).
 *   4 Rays.  h = (x T + y B) + z n per component;  vh = dot(v, h);  l_c = (2 vh) h_c - v_c;  w = dot(n, l).  The ray is
 *     VALID iff vh > 0 && w > 0; otherwise it is BELOW THE HORIZON (counts[3] += 1), is not traversed and adds +0.0 to every
 *     sum.  l is not normalised.
 *   5 Classification.  A valid ray (o, l) is traversed as in "Baking occlusion", 2 to 7 with t_max = max_distance (+inf: no
 *     limit) and classified as in "Baking light", 2: a miss, a FRONT hit (dot(l, n_g) < 0) or a BACK hit.
 *     counts[0..2] = misses, front hits, back hits.
 *   6 Radiance.  c of a miss is the sky texel of l ("Baking light", 3); of a front hit (b0 Q[i0] + b1 Q[i1]) + b2 Q[i2] with
 *     the float32-rounded weights of "Ray-traced light per point", 6 (0 if radiosity == NULL); of a back hit 0.
 *   7 Sums.  Lane i adds, for its rows in ascending chunk order from 0.0:  S_c += w c;  S_front_c += w c at a front hit (+0.0
 *     otherwise);  W += w;  W_miss += w at a miss (+0.0 otherwise).  All eight go through the butterfly of "Baking light", 5.
 *     specular[q] = float32(S / W), reflected[q] = float32(S_front / W) per channel, visibility[q] = float32(W_miss / W);
 *     W == 0 (no valid ray) gives 0, 0 and 1.  valid[q] = the valid rays, blocked[q] = those that hit any face.
 *   8 No cube.  With sky == NULL, specular and reflected are not touched (pass NULL); the rays are still traversed and
 *     classified, for visibility, valid, blocked and the counters: specular occlusion alone.
 * gigs_mesh_reflect_points, one one-wave block per row of `order` [N] int64 (the points sorted by cell, or NULL); counts [7]
 *   uint64 (cleared inside the call) = misses, front hits, back hits, rays below the horizon, no_normal points, no_view points,
 *   masked points.  sky_res = n in [1, 4096] when sky is given.  n_points == 0 launches nothing.
 * An order row, a cell_start entry, a pair key or a face index outside its range sets *overflow (cleared by the caller) and
 *   the wave stores nothing.
 * gigs_reflect_compose turns a radiance into the shade's specular_rgb, float32, one thread per point, no atomics: the lines
 *   of gigs_shade_fwd's specular term restated, every product and sum rounded on its own, in this order:
 *     nov = min(max((n_y v_y + n_z v_z) + n_x v_x, 1e-4), 1)
 *     fu = nov lut_w - 0.5, fv = roughness lut_h - 0.5;  tu = fu - floor(fu), tv = fv - floor(fv);  x0, x1 = floor(fu),
 *     floor(fu) + 1 and y0, y1 likewise, each clamped to the table;  lut [lut_h, lut_w, 2]
 *     fg = ((lut[y0,x0] (1-tu)(1-tv) + lut[y0,x1] tu (1-tv)) + lut[y1,x0] (1-tu) tv) + lut[y1,x1] tu tv
 *     F0_c = (1 - m) 0.04 + albedo_c m  (metallic == NULL: 0.04, and albedo is not read)
 *     specular_rgb_c = s_c (F0_c fg.x + fg.y),  s_c = radiance_c, or radiance_c visibility[q] when visibility is given
 *   normals, views, albedo, radiance, specular_rgb [N, 3], roughness, metallic, visibility [N] float32, mask [N] uint8 or
 *   NULL: a point with mask[q] == 0 gets 0. */
int gigs_mesh_reflect_points(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                             const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                             double scale, int n_points, const float* points, const float* normals, const float* views,
                             const float* roughness, const unsigned char* mask, const long long* order, const float* directions,
                             int n_levels, int n_rays, int n_rotations, unsigned long long seed, double max_distance, double bias,
                             int sky_res, const float* sky, const float* radiosity, float* specular, float* reflected,
                             float* visibility, int* valid, int* blocked, unsigned long long* counts, int* overflow,
                             void* stream);
int gigs_reflect_compose(int n_points, const float* normals, const float* views, const float* albedo, const float* roughness,
                         const float* metallic, const unsigned char* mask, const float* radiance, const float* visibility,
                         const float* lut, int lut_w, int lut_h, float* specular_rgb, void* stream);
/* Shadows of analytic lights (gigs-hip extension; the device half of mesh.shadow_points): for the points of "Ray-traced
 * light per point" and L point or directional lights, the share of each light's S samples that reach the point past the
 * mesh.  The conventions are that section's: DEVICE arrays except `lo` and `dims`, no synchronisation, no allocation,
 * float64 on the float32 inputs, + - * / only, no sqrt, no float atomics: tests/mesh_shadow_ref.py reproduces every bit.
 *   1 Lights.  lights [L, GIGS_LIGHT_ROW] float32, 1 <= L <= GIGS_MAX_LIGHTS; the caller keeps every entry finite.  Row l:
 *       [0]     kind: 0 a POINT light, anything else (1) a DIRECTIONAL light
 *       [1..3]  point: its position c;  directional: w, the unit direction the light TRAVELS in
 *       [4]     the extent e >= 0.  point: the radius of its sphere;  directional: the tangent of its half-angle
 *       [5..7]  0, reserved
 *   2 Offsets.  offsets [K, S, 3] float32, points of the unit ball, 1 <= S <= 64 samples, 1 <= K <= 64 rotations.
 *   3 Points.  Point q with mask[q] == 0 is MASKED (counts[4] += 1); otherwise a point that fails the no_normal rule of
 *     "Baking occlusion", 8 counts as no_normal (counts[3] += 1).  Either way no ray is cast, lit[q, :] = S and
 *     visibility[q, :] = 1.
 *   4 Rays.  o = p + bias n and k = mix((seed 2^32 + q) mod 2^64) mod K by the code of "Baking occlusion", 8.  For light l and
 *     sample s let u = offsets[k, s] and, per component,
 *       point:        d = (c + e u) - o,  t_max = 1             (the sample of the sphere lies at t = 1)
 *       directional:  d = (-w) + e u,     t_max = max_distance  (+inf: no limit)
 *   5 Classification.  The sample is BELOW THE HORIZON if !(dot(d, n) > 0) -- d = 0 and a NaN as well -- and then no ray is
 *     cast (counts[2] += 1).  Otherwise a ray is cast (counts[0] += 1) and the sample is BLOCKED iff the ray has an accepted
 *     face within t_max ("Baking occlusion", 2 to 7): iff the nearest-face traversal would find one (counts[1] += 1).  The
 *     kernel's walk returns at the first accepted face; DESIGN.md, "Analytic lights and shadows", proves the two agree.
 *   6 lit[q, l] = the samples that are neither; visibility[q, l] = float32(double(lit) / double(S)).
 * gigs_mesh_shadow_points, one thread per (row of `order` [N] int64 -- the points sorted by cell, or NULL --, light, sample),
 *   flattened in that order over one-wave blocks; lit [N, L] int32 is cleared inside the call and counted with integer
 *   atomics, a second launch stores visibility [N, L] float32.  counts [5] uint64 (cleared inside the call) = rays cast,
 *   blocked, below the horizon, no_normal points, masked points.  n_points == 0 launches nothing.
 * An order row, a cell_start entry, a pair key or a face index outside its range sets *overflow (cleared by the caller) and
 *   the thread adds nothing. */
#define GIGS_LIGHT_ROW 8
int gigs_mesh_shadow_points(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                            const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                            double scale, int n_points, const float* points, const float* normals, const unsigned char* mask,
                            const long long* order, int n_lights, const float* lights, const float* offsets, int n_samples,
                            int n_rotations, unsigned long long seed, double bias, double max_distance, int* lit,
                            float* visibility, unsigned long long* counts, int* overflow, void* stream);
/* Shading under analytic lights (gigs-hip extension; the device half of analytic_lights.shade_lights): the points of the
 * section above under its L lights, Lambert plus GGX with Smith-correlated masking and Schlick Fresnel -- the arithmetic of
 * the reference's pbr/renderutils/bsdf.py bsdf_pbr(kd = albedo, arm = (0, roughness, metallic), pos = p, nrm = n,
 * view_pos = campos, light_pos = p + wi, min_roughness = 0.08, BSDF = 0), which the reference never calls.  float32, one
 * thread per point, DEVICE arrays, no synchronisation, no allocation, no atomics.  eps = 1e-4 (specular_epsilon),
 * clamp(c) = min(max(c, eps), 1 - eps), normalize(v) = v / max(|v|, 1e-12).
 *   1 Points.  A point with mask[q] == 0 or one that fails the no_normal rule (float64, as above) gets zeros.
 *   2 Material.  m = metallic[q] (NULL: 0); ks = 0.04 (1 - m) + albedo m; kd = albedo (1 - m); alpha = min(max(roughness^2,
 *     0.08^2), 1); a2 = alpha^2; wo = normalize(campos - p).
 *   3 Per light l = 0 .. L - 1, in this order; E_l = radiance[l] (colour x intensity), vis = visibility[q, l] (NULL: 1):
 *       point:        v = c - p;  wi = v / sqrt(v.v);  E = E_l / max(v.v, 1e-8)
 *       directional:  wi = -w;                         E = E_l
 *     h = normalize(wo + wi);  D = a2 / (d d pi) with c = clamp(n.h), d = (c a2 - c) c + 1;
 *     Lambda(x) = 0.5 (sqrt(1 + a2 (1 - c c) / (c c)) - 1) with c = clamp(x);  G = 1 / (1 + Lambda(n.wo) + Lambda(n.wi));
 *     F = ks + (1 - ks) f^5 with f = 1 - clamp(wo.h), f^5 = ((f f)(f f)) f;
 *     spec = F D G 0.25 / max(n.wo, eps) if n.wo > eps and n.wi > eps, else 0.  Both terms carry the cosine n.wi:
 *       diffuse[q]  += (vis E) (kd max(n.wi, 0) / pi)          (a NaN n.wi, a light at the point itself, gives 0)
 *       specular[q] += (vis E) spec
 *     from 0, so two lights give the float32 sum of the two single results.
 * Outputs diffuse, specular [N, 3] float32, linear radiance.  1 <= L <= GIGS_MAX_LIGHTS.  n_points == 0 launches nothing. */
int gigs_shade_lights(int n_points, const float* points, const float* normals, const unsigned char* mask, const float* albedo,
                      const float* roughness, const float* metallic, const float* campos, int n_lights, const float* lights,
                      const float* radiance, const float* visibility, float* diffuse, float* specular, void* stream);
/* Denoising ray-traced planes (gigs-hip extension; the device half of denoise.atrous): an edge-avoiding a-trous wavelet
 * filter in the manner of Dammertz 2010 and SVGF, single frame, over the planes the per-pixel tracers return, guided by
 * their prepared points and normals.  DEVICE arrays except `groups`, no synchronisation, no allocation, no atomics.
 * float32, + - * / only, built with -ffp-contract=off: every product and sum below is rounded on its own, in the order the
 * brackets give.  No exp, pow or sqrt: every edge-stopping function is a polynomial of compact support, so a weight across a
 * real edge is exactly 0 and tests/denoise_ref.py reproduces every bit in numpy float32.  max(a, b) is (a > b) ? a : b.
 *   1 Inputs.  signal [C, H, W] float32, 1 <= C <= GIGS_DENOISE_MAX_CHANNELS.  groups [G] int (HOST): channel counts, each 1
 *     or 3, summing to C; the channels of a group are consecutive and share one weight.  The VALUE of a group at a pixel is
 *     y = x_0, or (x_0 + x_1) + x_2.  points, normals [H W, 3] float32 and mask [H W] uint8 are the prepared arrays of
 *     "Ray-traced light per point", row-major over the pixels; roughness [H W] float32 or NULL.
 *   2 Live pixels.  A pixel is LIVE iff its mask is non-zero and its 6 guide components, its roughness (if given) and its C
 *     signal values are all finite (|v| <= FLT_MAX).  A pixel that is not live keeps the bits of its input, is skipped as
 *     a tap everywhere, and has variance 0.
 *   3 Geometry weight of tap q seen from centre p (P the point, N the normal, r the roughness):
 *       c   = (Np.x Nq.x + Np.y Nq.y) + Np.z Nq.z;  c = max(c, 0);  then c = c c, e times    (normal_power = 2^e, 0 <= e <= 7)
 *       d   = ((Pq.x - Pp.x) Np.x + (Pq.y - Pp.y) Np.y) + (Pq.z - Pp.z) Np.z         (q's distance from p's tangent plane)
 *       z   = max(1 - (d d) inv_plane2, 0)                   (inv_plane2 = float32(1 / plane_distance^2), made on the host)
 *       g   = c (z z)
 *       with a roughness guide:  t = rq - rp;  u = max(1 - (t t) inv_rough2, 0);  g = g (u u)
 *   4 Launch A, the variance (gigs_denoise_variance).  For a live pixel p and each group, over the live taps q of the 5 x 5
 *     window of step 1 that lie inside the image, in row-major order, every sum started at 0:
 *       G = sum g;   T = sum (g (y_q - y_p));   if !(G > 0): var = 0, else
 *       m = y_p + T / G;   U = sum (g ((y_q - m) (y_q - m)));   var = U / G
 *     Two passes, not E[y^2] - m^2, and the mean in the difference form of 5: (sum g y_q) / G of a constant y is y only up to
 *     rounding, y_p + 0 / G is y, so a constant signal has variance exactly 0.  (G = 0 needs a centre whose normal has no
 *     length: such a pixel weighs nothing.)
 *   5 Launches B_i, i = 0 .. n - 1 (gigs_denoise_atrous), step s = 2^i <= GIGS_DENOISE_MAX_STEP.  Taps at the offsets
 *     {-2s, -s, 0, s, 2s} in y (outer) and x (inner), h = (1/16, 1/4, 3/8, 1/4, 1/16); taps outside the image and taps that
 *     are not live are skipped, the centre is a tap.  For a live pixel p and group j, sums started at 0, taps row-major:
 *       r     = 1 / (sigma_l2 var_p + eps)                  (eps > 0; sigma_l2 = 0 with eps = +inf gives r = 0: the signal
 *                                                            weight is off)
 *       delta = y_q - y_p;   l = max(1 - (delta delta) r, 0);   w = ((h[dy] h[dx]) g) (l l)
 *       Wsum += w;   D_c += w (x_q,c - x_p,c) for each channel c of the group;   V += (w w) var_q
 *       if Wsum > 0:  x'_p,c = x_p,c + D_c / Wsum,  var'_p = V / (Wsum Wsum);   otherwise x' = x and var' = var.
 *     The difference form returns a constant signal with its own bits.  `/` is the correctly rounded float32 division.
 *   6 Layout.  gigs_denoise_pack writes pixel-major records: guide [H W, 8] float32 = (P, N, roughness or 0, live ? 1 : 0)
 *     and record [H W, S] float32, S = 4 ceil((C + G) / 4) = (the C values, G variances (0), padding (0)).
 *     gigs_denoise_variance and gigs_denoise_atrous read one record array and write ANOTHER (record_in != record_out; the
 *     caller owns the ping-pong pair); gigs_denoise_unpack writes filtered [C, H, W] and variance [G, H, W] from a record
 *     array.  The filter launches take 16 x 16 pixels of one sub-lattice (x mod s, y mod s) per 256-thread block and stage the
 *     20 x 20 records around them in 400 (8 + S) 4 <= 64000 bytes of LDS.  Nothing outside [0, H) x [0, W) is read.
 * H W = 0 launches nothing.  Refused: C, G or a group outside its range, groups that do not sum to C, H W > 2^31 - 1, e
 *   outside [0, 7], a step that is no power of two in [1, GIGS_DENOISE_MAX_STEP], inv_plane2, inv_rough2 or sigma_l2 negative,
 *   NaN or infinite, eps <= 0 or NaN, record_in == record_out, a NULL array. */
#define GIGS_DENOISE_MAX_CHANNELS 16
#define GIGS_DENOISE_MAX_STEP 16
int gigs_denoise_pack(int width, int height, int channels, int n_groups, const int* groups, const float* signal,
                      const float* points, const float* normals, const unsigned char* mask, const float* roughness,
                      float* guide, float* record, void* stream);
int gigs_denoise_variance(int width, int height, int channels, int n_groups, const int* groups, int normal_exponent,
                          float inv_plane2, int use_roughness, float inv_rough2, const float* guide, const float* record_in,
                          float* record_out, void* stream);
int gigs_denoise_atrous(int width, int height, int channels, int n_groups, const int* groups, int step, int normal_exponent,
                        float inv_plane2, int use_roughness, float inv_rough2, float sigma_l2, float eps, const float* guide,
                        const float* record_in, float* record_out, void* stream);
int gigs_denoise_unpack(int width, int height, int channels, int n_groups, const int* groups, const float* record, float* filtered,
                        float* variance, void* stream);
/* Texturing meshes (gigs-hip extension; the device half of mesh.bake_atlas / mesh.transfer_attributes): the per-vertex
 * channels of a heavy SOURCE mesh stored in the texels of an atlas over a light TARGET mesh.  Every texel of the atlas gets
 * the point of the target's surface it stands for (gigs_mesh_atlas_points), the search of "Comparing meshes" finds the
 * source face closest to that point (gigs_mesh_closest), and gigs_mesh_transfer finds WHERE on that face the closest point
 * lies and interpolates the channels there.  All arrays are DEVICE memory; the calls neither synchronise nor allocate.  One
 * independent thread per texel or query, no float atomics, no thread waits on another.  All arithmetic is float64 on the
 * float32 inputs, + - * / only, every product and sum rounded on its own (dot and cross as under "Comparing meshes"): no
 * sqrt, no transcendental, so tests/mesh_atlas_ref.py reproduces every bit in numpy.
 *   1 Blocks.  B = block >= 3.  A block is (B + 1) x B texels (wide x high) and holds two faces: face f lies in block
 *     f / 2, half f % 2.  Texel (i, j) of a block, 0 <= i <= B, 0 <= j <= B - 1, belongs to the LOWER half (0) if
 *     i + j <= B - 1, else to the UPPER half (1); each half owns B (B + 1) / 2 texels.  The upper half is the point
 *     reflection (i, j) -> (B - i, B - 1 - j) of the lower: an upper texel takes the lower half's formulas at its reflected
 *     coordinates (li, lj); a lower texel has (li, lj) = (i, j).
 *   2 Image.  per_row = W / (B + 1) blocks to a row (integer division, per_row >= 1), block b at column b % per_row and
 *     row b / per_row: its texel (i, j) is the image texel x = (b % per_row)(B + 1) + i, y = (b / per_row) B + j, row y
 *     counted from the TOP of the image, and dest = y W + x.  H = ceil(n_blocks / per_row) B, n_blocks = ceil(F / 2).
 *     mesh.atlas_layout's default W is the smallest power of two >= B + 1 with (W / (B + 1)) (W / B) >= n_blocks.  The
 *     columns right of the last whole block, the slots past F and the texels of an unusable face are UNBAKED: value 0,
 *     coverage 0.
 *   3 UV.  The centre of texel (x, y) is the point (x + 1/2, y + 1/2) in texel coordinates.  Corner k of a face sits at the
 *     centre of a texel of its half: lower (0, 0), (B - 2, 0), (0, B - 2); upper (B, B - 1), (2, B - 1), (B, 1).  uv =
 *     (float32(X / W), float32(1 - Y / H)) for the point (X, Y) in texel coordinates: v = 0 is the BOTTOM row of the image
 *     (the OBJ convention), kept by scene_io.save_mesh_obj and mesh.sample_atlas.  For every point of a face's UV
 *     triangle, edges and corners included, every bilinear tap of non-zero weight is a texel of that face's half.
 *   4 Texel to point.  w1 = li / (B - 2), w2 = lj / (B - 2), w0 = (1 - w1) - w2; point = float32((w0 p0 + w1 p1) + w2 p2)
 *     per component, bary = (float32(w1), float32(w2)).  The texels with li + lj = B - 1 lie outside the UV triangle: w0 =
 *     -1 / (B - 2), and the point is the EXTRAPOLATED one of the face's plane.  That is the gutter; there is no dilation.
 *     texel_face = f, or -1 for a slot past F.  For a slot past F, a face with an index outside [0, V) or a non-finite
 *     corner: dest = -1 and point = NaN in every component (gigs_mesh_closest then answers face -1).  A face without area
 *     is baked like any other.
 *   5 Closest point on a given face (i0, i1, i2), corners p0, p1, p2.  The candidates, expressions and order of 5 of
 *     "Comparing meshes": edge 01, edge 12, edge 20, each walked from the vertex with the lower INDEX with s = 0 for
 *     t <= 0, s = 1 for t >= den, else s = t / den, and the same d^2; the weights are (1 - s, s) on the edge's ends in the
 *     walking direction and 0 on the third vertex.  Then, if the three edge functions f0 over (p0, p1), f1 over (p1, p2),
 *     f2 over (p2, p0) are >= 0, the interior with d^2 = dot(p - p0, n)^2 / dot(n, n) and the weights (w0, w1, w2) =
 *     (f1 / S, f2 / S, f0 / S), S = (f0 + f1) + f2 (the raycast's W); it is taken only with S > 0.  A later candidate wins
 *     only with a strictly smaller d^2.
 *   6 Transfer.  values [V, C] float32, 1 <= C <= 16: out[c] = float32((w0 a0[c] + w1 a1[c]) + w2 a2[c]) with a_k the row
 *     of vertex i_k; bary = (float32(w1), float32(w2)).  With `dest` [N] int64, out is C planes of `plane` floats, the
 *     query stores at out[c plane + dest[q]] and sets coverage[dest[q]] = 1; without it, out is [N, C] and coverage is
 *     not used.  A query with face -1 or dest -1, a non-finite query point or a non-finite corner stores nothing (the
 *     caller zero-fills) and counts[1] += 1; every other query counts[0] += 1.
 * gigs_mesh_atlas_points, one thread per texel of the n_blocks blocks, block-major: q = b B (B + 1) + j (B + 1) + i gets
 *   points [Q,3], bary [Q,2], texel_face [Q], dest [Q] int64 as in 4.  3 <= block <= 1024, Q < 2^31.  A texel outside the
 *   W x H image sets *overflow.  n_blocks == 0 launches nothing.
 * gigs_mesh_transfer, one thread per query: out, coverage, bary [N,2] as in 5 and 6; counts [2] uint64 (cleared inside the
 *   call; integer atomics) = transferred, skipped.  A face >= F or < -1, a dest outside [-1, plane) or a vertex index
 *   outside [0, V) sets *overflow (device int, cleared by the caller) and the thread stores nothing. */
int gigs_mesh_atlas_points(int n_vertices, int n_faces, const float* vertices, const int* faces, int block, int width, int height,
                           int n_blocks, float* points, float* bary, int* texel_face, long long* dest, int* overflow,
                           void* stream);
int gigs_mesh_transfer(int n_vertices, int n_faces, const float* vertices, const int* faces, int n_channels, const float* values,
                       int n_points, const float* points, const int* face, const long long* dest, long long plane, float* out,
                       unsigned char* coverage, float* bary, unsigned long long* counts, int* overflow, void* stream);
/* Rendering meshes (gigs-hip extension; the device half of mesh_render.py): a triangle mesh -- vertices [V,3], faces [F,3]
 * int32 and mesh.py's per-vertex attributes -- as the G-buffer planes the blend kernel writes in inference mode, by a
 * visibility buffer.  Coverage and visibility are integer decisions, so no result depends on the order of execution and a
 * restatement (tests/mesh_raster_ref.py) agrees index for index.  All arrays are DEVICE memory, viewmatrix included (the
 * rasterizer's layout); the calls neither synchronise nor allocate.  Every product and sum is rounded on its own, division
 * is IEEE.  There is NO clipping: a triangle with a flagged vertex is dropped whole.
 * gigs_mesh_project, one thread per vertex:
 *     p = xform_point_4x3(vertex, viewmatrix);  u = p.x / p.z * fx + (W - 1) / 2, v = p.y / p.z * fy + (H - 1) / 2 with
 *     fx = W / (2 tanfovx), fy = H / (2 tanfovy): gigs_tsdf_integrate's pixel convention, pixel centres at the integers.
 *     view_pos [V,3] = p;  screen [V,2] = (X, Y) = (rint(256 u), rint(256 v)), round half to even;  flags [V] = 1 where
 *     p.z <= 0.2 (the rasterizer's near cull), where p.x, p.y, p.z, u or v is not finite, or where |u| or |v| exceeds
 *     16384 pixels (the guard band), else 0.  A flagged vertex gets screen = (0, 0).
 * gigs_mesh_raster: vis [H,W] of 64-bit keys, set to all ones by the CALLER, receives per pixel the minimum of
 *     key = (bits(z) << 32) | triangle index  over the triangles that cover the pixel's centre.
 *   Dropped, without a memory access through a bad index: a triangle with a vertex index outside [0, V), with a flagged
 *     vertex, or with doubled area A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) == 0 (int64).  If A < 0, vertices 1 and 2
 *     swap roles (and A changes sign) in everything below.
 *   Coverage at the centre q = (256 i, 256 j) of pixel (i, j): the int64 edge functions E0 over the edge 1 -> 2, E1 over
 *     2 -> 0, E2 over 0 -> 1, each (Xb - Xa)(qy - Ya) - (Yb - Ya)(qx - Xa).  The pixel is covered iff for every edge
 *     E > 0, or E == 0 and the directed edge (dx, dy) = (Xb - Xa, Yb - Ya) has dy < 0 || (dy == 0 && dx > 0): a centre on
 *     an edge two triangles share belongs to exactly one of them.
 *   Depth: b_k = float(E_k) / float(A) (int64 -> fp32 to nearest), w_k = b_k * (1 / z_k) with z_k = view_pos[vertex k].z,
 *     s = (w0 + w1) + w2, z = 1 / s; a z that is not finite or not above 0 is skipped.
 *   A triangle whose box of pixel centres, clamped to the image, holds at most small_max pixels (a negative value means
 *     GIGS_MESH_SMALL_MAX) is walked by its own thread; a larger one is appended to a device list and walked by a second
 *     launch, one wave per triangle, whose fixed grid strides over the device-side count (no read-back).  Both paths and
 *     every small_max give the same bits.  scratch: gigs_mesh_raster_scratch_bytes(F) bytes (the counter and the list),
 *     cleared inside the call.
 * gigs_mesh_resolve, one thread per pixel: the triangle index of the pixel's key is range-checked against F and the
 *   triangle set up and sampled again by the same device function, so depth has the bits of the key.  Planes as
 *   the blend kernel's ([C,H,W]): opacity = 1, depth = z, pos = ((w0 x0 + w1 x1) + w2 x2) / s per component of view_pos,
 *   normal, albedo, roughness, metallic interpolated the same way (the normal is not renormalised), normal_view =
 *   normalize3(xform_vec_4x3(normal, viewmatrix)), tri_id [H,W] int32 = the triangle.  A pixel with an empty key gets what
 *   the blend kernel writes where no Gaussian contributes under a black background with inference = 1: zeros,
 *   roughness = 1, normal_view = normalize3 of the zero vector (NaN), and tri_id = -1.
 * gigs_mesh_resolve_textured, one thread per pixel: gigs_mesh_resolve for a mesh whose materials live in a texture atlas
 *   (mesh.bake_atlas's planes, texture_mesh.py's images) instead of per-vertex tables.  The same device functions set the
 *   triangle up and sample it, so tri_id, opacity, depth and pos have the bits gigs_mesh_resolve gives on the same key
 *   plane.  uvs [F,3,2] float32 holds one UV per face CORNER and is indexed by the triangle alone (no second index table);
 *   tex_albedo, tex_orm (occlusion, roughness, metallic) and tex_normal are planes [3,Ht,Wt] float32, 1 <= Wt, Ht <= 16384;
 *   tex_normal holds the world normal as interpolated, not normalised, and may be NULL: then `normals` [V,3] is
 *   interpolated exactly as in gigs_mesh_resolve (it is not read otherwise and may be NULL).  Every operation is rounded on
 *   its own, in float32:
 *     Corners.  Where the set-up swapped vertices 1 and 2 (A < 0) the corner UVs swap with them: uv_k is the UV of the
 *       corner that became vertex k.
 *     u = ((w0 u_0 + w1 u_1) + w2 u_2) / s, v likewise (perspective-correct, as every attribute).
 *     x = u Wt - 0.5, y = (1 - v) Ht - 0.5: v = 0 is the BOTTOM row of the image (the OBJ convention, mesh.sample_atlas's
 *       formulas).  x = fminf(fmaxf(x, -1), Wt), y = fminf(fmaxf(y, -1), Ht); fmaxf returns its non-NaN argument, so a NaN
 *       coordinate becomes -1 and no conversion to int is out of range.
 *     x0 = floorf(x), fx = x - x0, xa = clamp(int(x0), 0, Wt - 1), xb = clamp(int(x0) + 1, 0, Wt - 1); y0, fy, ya, yb
 *       likewise.
 *     Per channel of a plane t: (1 - fy) ((1 - fx) t[ya,xa] + fx t[ya,xb]) + fy ((1 - fx) t[yb,xa] + fx t[yb,xb]).
 *   There are no mips and no coverage test: an unbaked texel reads as the 0 it holds.  Planes: the eight of
 *   gigs_mesh_resolve -- albedo, roughness, metallic from the textures, normal from tex_normal (or the vertex normals),
 *   normal_view = normalize3(xform_vec_4x3(normal, viewmatrix)) -- plus occlusion [1,H,W], the O channel, and tri_id.  An
 *   empty key gives gigs_mesh_resolve's background and occlusion = 1 (open).
 * Images up to 16384 x 16384. */
#define GIGS_MESH_SMALL_MAX 64
int gigs_mesh_project(int n_vertices, const float* vertices, const float* viewmatrix, float tanfovx, float tanfovy, int width,
                      int height, float* view_pos, int* screen, uint8_t* flags, void* stream);
size_t gigs_mesh_raster_scratch_bytes(int n_faces);
int gigs_mesh_raster(int n_vertices, int n_faces, const int* faces, const float* view_pos, const int* screen,
                     const uint8_t* flags, int width, int height, int small_max, unsigned long long* vis, void* scratch,
                     void* stream);
int gigs_mesh_resolve(int n_vertices, int n_faces, const int* faces, const float* view_pos, const int* screen,
                      const uint8_t* flags, const float* normals, const float* albedo, const float* roughness,
                      const float* metallic, const float* viewmatrix, int width, int height, const unsigned long long* vis,
                      float* opacity, float* depth, float* pos, float* normal, float* normal_view, float* albedo_out,
                      float* roughness_out, float* metallic_out, int* tri_id, void* stream);
int gigs_mesh_resolve_textured(int n_vertices, int n_faces, const int* faces, const float* view_pos, const int* screen,
                               const uint8_t* flags, const float* uvs, const float* normals, int tex_width, int tex_height,
                               const float* tex_albedo, const float* tex_orm, const float* tex_normal, const float* viewmatrix,
                               int width, int height, const unsigned long long* vis, float* opacity, float* depth, float* pos,
                               float* normal, float* normal_view, float* albedo_out, float* roughness_out, float* metallic_out,
                               float* occlusion_out, int* tri_id, void* stream);
int gigs_tv_loss_fwd(int channels, int height, int width, int step, const float* gt, const float* prediction,
                     const float* mask_f, float* scratch, float* loss, void* stream);
int gigs_tv_loss_bwd(int channels, int height, int width, int step, const float* gt, const float* prediction,
                     const float* mask_f, const float* g_loss, float* g_prediction, void* stream);
int gigs_masked_l1_fwd(int channels, int height, int width, const float* a, const float* b, const uint8_t* mask,
                       float* scratch, float* loss_count, void* stream);
int gigs_masked_l1_bwd(int channels, int height, int width, const float* a, const float* b, const uint8_t* mask,
                       const float* loss_count, const float* g_loss, float* g_a, float* g_b, void* stream);
int gigs_adam_step(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                   void* stream);
/* hipGraph-capturable form (gigs-hip extension): the per-step scalars of group k -- {lr / (1 - beta1^t), sqrt(1 - beta2^t)}
 * -- are read by the kernel from DEVICE memory, dyn[2k], dyn[2k+1] (k = index into `groups`; the groups' lr / step members
 * are ignored), so a captured launch stays valid while the host refreshes the table before every replay.
 * gigs_adam_scalars computes one group's pair exactly as gigs_adam_step does (double arithmetic, torch's order). */
int gigs_adam_step_dyn(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                       const float* dyn, void* stream);
void gigs_adam_scalars(double lr, int step, double beta1, double beta2, float* out2);
/* gigs_adam_step_dyn that also reports whether the update CHANGED a bit of any watched group: `watch` is a HOST array of
 * n_groups flags (non-zero = watched), `changed` a DEVICE word that is OR-ed with 1 when a parameter of a watched group
 * differs from its value before the step (it is never cleared here).  A stage-2 trainer watches the geometry groups: as
 * long as the word stays 0, per-view tile lists, occlusion planes and indirect-light hit lists remain valid
 * (gigs_ctx_set_reuse_binning). */
int gigs_adam_step_watch(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                         const float* dyn, const unsigned char* watch, unsigned* changed, void* stream);
/* gigs_adam_step_watch behind a guard: `guard` is a DEVICE word (NULL = none); while it is non-zero the launch changes nothing
 * -- parameters, moments and gradients stay as they are.  With the violation counter of gigs_ctx_set_materials_only as the
 * guard, an update is never computed from gradients that were taken for zero and were not. */
int gigs_adam_step_guarded(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                           const float* dyn, const unsigned char* watch, unsigned* changed, const unsigned* guard, void* stream);

/* The parameter getters of GaussianModel (scene/gaussian_model.py:48-58, 178-263) as one pass each way:
 * shs = cat(f_dc [P,1,3], f_rest [P,K-1,3]) -> [P,K,3]; opacities / albedo / roughness / metallic = sigmoid(raw);
 * scales = exp(scaling); rotations = F.normalize(rotation), normal = F.normalize(normal) (dim -1, eps 1e-12).
 * gigs_activate_fwd: out->shs may be NULL (the caller hands the two SH tensors to the rasterizer as they are:
 * gigs_ctx_set_split_sh) -- no concatenation then.
 * gigs_activate_bwd: grad_out members may be NULL (= zero gradient); every non-NULL grad_raw tensor is overwritten, a NULL
 * one is neither computed nor written (a gradient the caller knows to be zero and keeps no tensor for). */
typedef struct gigs_activation_raw {
  const float *f_dc, *f_rest, *opacity, *normal, *albedo, *roughness, *metallic, *scaling, *rotation;
} gigs_activation_raw;
typedef struct gigs_activation_out { /* forward: outputs; backward: their incoming gradients */
  float *shs, *opacities, *normal, *albedo, *roughness, *metallic, *scales, *rotations;
} gigs_activation_out;
typedef struct gigs_activation_raw_grad {
  float *f_dc, *f_rest, *opacity, *normal, *albedo, *roughness, *metallic, *scaling, *rotation;
} gigs_activation_raw_grad;
int gigs_activate_fwd(int P, int K, const gigs_activation_raw* raw, const gigs_activation_out* out, void* stream);
int gigs_activate_bwd(int P, int K, const gigs_activation_raw* raw, const gigs_activation_out* grad_out,
                      const gigs_activation_raw_grad* grad_raw, void* stream);

/* Densification bookkeeping (gigs-hip extension).
 * gigs_densify_stats = train.py:494-498 + GaussianModel.add_densification_stats (scene/gaussian_model.py:933-945) in one
 *   pass over the P Gaussians, for those with radii > 0: max_radii2D = max(., radii); xyz_gradient_accum += |(gx,gy)|;
 *   xyz_gradient_accum_abs += |gx|+|gy|; xyz_gradient_accum_abs_max = max(., |gx|+|gy|); denom += 1.
 *   viewspace_grad is means2D.grad [P,3]; the five statistics are fp32 [P].
 * gigs_gather_rows rebuilds any number of row-major fp32 tensors after a densify / prune decision in one launch
 *   (replaces the per-tensor boolean-mask indexing and torch.cat of scene/gaussian_model.py:595-706):
 *   dst_t[r, :] = (zero_row && zero_row[r] && t.zero_new) ? 0 : src_t[src_index[r], :] for r < n_rows_out;
 *   src_index values must lie in [0, n_rows_in): the kernel does not check them (gi-gs_amd/densify.py builds them from
 *   arange(n_rows_in) selections only). */
typedef struct gigs_gather_tensor {
  const float* src;
  float* dst;
  int row_floats; /* floats per row */
  int zero_new;   /* 1: rows flagged in zero_row become zero (optimizer moments of new Gaussians) */
} gigs_gather_tensor;
int gigs_densify_stats(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum,
                       float* xyz_gradient_accum_abs, float* xyz_gradient_accum_abs_max, float* denom,
                       float* max_radii2D, void* stream);
/* The same with a device guard: nothing is added while *skip != 0 (skip = NULL: unguarded).  Captured behind a
 * forward under asynchronous binning with skip = its overflow counter, a replay whose binning overflowed -- and that
 * the caller repeats -- leaves the statistics untouched (gi-gs_amd/pipeline.py: WholeStepGraph). */
int gigs_densify_stats_guarded(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum,
                               float* xyz_gradient_accum_abs, float* xyz_gradient_accum_abs_max, float* denom,
                               float* max_radii2D, const int* skip, void* stream);
int gigs_gather_rows(int n_tensors, const gigs_gather_tensor* tensors, long long n_rows_out, long long n_rows_in,
                     const int* src_index, const uint8_t* zero_row, void* stream);

/* simple-knn's distCUDA2 (submodules/simple-knn/simple_knn.cu:165-224, ext.cpp / spatial.cu):
 * mean_dists[i] = mean of the squared distances from points[i] to its three nearest other points (by index: duplicates
 * count, at distance 0); with fewer than four points the reference's FLT_MAX placeholders stay in the sum (> 1e38 or +inf).  points [P,3] fp32.
 * scratch: gigs_dist2_scratch_bytes(P) bytes of device memory.  No host read-back; everything is queued on `stream`. */
size_t gigs_dist2_scratch_bytes(int P);
int gigs_dist2(int P, const float* points, float* mean_dists, void* scratch, size_t scratch_bytes, void* stream);

/* Test/diagnostic views into the opaque scratch buffers (byte offsets from the buffer
 * start, or -1).  `which`: geometry 0 depths f32[P], 1 pos_view f32[3P], 2 means2D f32[2P],
 * 3 cov3D f32[6P], 4 conic_opacity f32[4P], 5 rgb f32[3P], 6 clamped u8[3P],
 * 7 tiles_touched u32[P], 8 point_offsets u32[P];  binning 0 keys_unsorted u64[R],
 * 1 values_unsorted u32[R], 2 keys u64[R], 3 point_list u32[R], 4 hit_mask u8[4][R] (byte i of plane w: quadrant
 * w of instance i's tile blended it);  image 0 final_T f32[N],
 * 1 n_contrib u32[N], 2 ranges u32[2T], 3 tile_order u32[T] (the blend kernels' workgroup -> tile map, longest lists first). */
long long gigs_geom_offset(int P, int which);
long long gigs_binning_offset(int num_rendered, int which);
long long gigs_image_offset(int width, int height, int which);

/* Self-test of two exact rewrites used by the SSAO/SSR march: out_fast[2i..] = the shared-reciprocal
 * division (nx[i]/d[i], ny[i]/d[i]), out_ref = the same with the compiler's IEEE division;
 * out_round[2i] = the add-and-truncate rounding of nx[i], out_round[2i+1] = (int)roundf(nx[i]). */
int gigs_selftest_div2(int n, const float* nx, const float* ny, const float* d, float* out_fast,
                       float* out_ref, int* out_round, void* stream);
/* Exhaustive self-test of the march's pixel rounding: *mismatches (device u64) receives the number of fp32 bit
 * patterns t (all 2^32 are tried) for which floor(t + (0.5 - 2^-25)) and (int)roundf(t) would select a different
 * pixel or decide "inside the image" differently for some image side < 2^15.  Expected: 0. */
int gigs_selftest_round(unsigned long long* mismatches, void* stream);

/* Rasterizer::lite_forward (R/cuda_rasterizer/rasterizer.h:90-117; bound as _C.lite_rasterize_gaussians,
 * R/rasterize_points.cu:39-127): colour [3,H,W], opacity [1,H,W] and depth [1,H,W] only, "for baking".  Composites exactly
 * like gigs_forward; the geometry / image callbacks are asked for somewhat more than gigs_required_geom / _image
 * (zero material attributes and the planes that are not returned live there).  Returns num_rendered. */
int gigs_lite_forward(gigs_ctx* ctx, gigs_alloc_fn geometryBuffer, void* geom_user, gigs_alloc_fn binningBuffer, void* binning_user,
                      gigs_alloc_fn imageBuffer, void* image_user, int P, int D, int M, const float* background, int width,
                      int height, const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                      const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                      const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                      int prefiltered, int argmax_depth, float* out_color, float* out_opacity, float* out_depth, int* radii,
                      int debug, void* stream);

/* The backward of Gaussian_SSR as the reference's autograd function defines it (R/diff_gaussian_rasterization/__init__.py:
 * 671-693): grad_albedo [3,H,W] = grad_color * abd; roughness / metallic / F0 receive nothing.  (The reference also exports
 * a CUDA SSR_BACKWARD whose only call is commented out; this entry is the live arithmetic, not that kernel.) */
int gigs_ssr_backward(int width, int height, const float* grad_color, const float* abd, float* grad_albedo, void* stream);

/* Frozen geometry (gigs-hip extension).  A stage-2 iteration of train.py updates materials and light only
 * (train.py:330-420): positions, covariances and opacities -- hence every tile list -- are the same from one visit of a
 * view to the next.  After gigs_ctx_set_reuse_binning(ctx, 1) a gigs_forward(ctx, ...) runs the preprocess (the per-Gaussian
 * records carry the material attributes) and the blend, and SKIPS count / prefix / scatter / sort: the binning and image
 * chunks its callbacks return must still hold what an earlier forward of the SAME view and geometry left there (ranges,
 * tile order, sorted point list; asynchronous layout: needs gigs_ctx_set_async_binning with the same capacity).  Outputs
 * are then those of a complete forward bit for bit.  Whether the geometry is unchanged is the caller's knowledge
 * (gigs_adam_step_watch reports it from the optimizer step). */
int gigs_ctx_set_reuse_binning(gigs_ctx* ctx, int on);

/* Declared stage-2 gradient set (gigs-hip extension).  The loss of a stage-2 iteration reaches the material planes and
 * the light only (train.py:330-420), and the material planes' blend gradients do not feed dL/dalpha (backward.cu:580-590):
 * every gradient of gigs_backward other than dL_dalbedo / dL_droughness / dL_dmetallic (and the densification slot of
 * dL_dmean2D) is an exact zero, 59 of 67 floats per Gaussian at SH degree 3 that the reference writes, activates and feeds
 * to Adam all the same.  After gigs_ctx_set_materials_only(ctx, violations) -- `violations` a DEVICE uint32 the caller
 * zeroes -- gigs_backward(ctx, ...) writes those four outputs only; every other gradient pointer may be NULL and is never
 * written.  The premise is checked on the device: each wave that finds a live Gaussian whose blend-backward record holds a
 * non-zero (or NaN) value in any other slot adds 1 to *violations; a caller that reads a non-zero count has used zeros that
 * were not zeros and must not continue.  The consumers take the absent gradients as what they are: gigs_activate_bwd skips a
 * NULL grad_raw member, a gigs_adam_group with grad == NULL is updated with g = 0 (same arithmetic, nothing read).
 * violations == NULL restores the complete backward. */
int gigs_ctx_set_materials_only(gigs_ctx* ctx, void* violations);

/* Split SH input (gigs-hip extension).  The optimizer keeps the SH coefficients as two tensors -- _features_dc [P,1,3] and
 * _features_rest [P,M-1,3] (scene/gaussian_model.py:48-58) -- and get_features concatenates them for every render: a pure copy
 * of 12 M bytes per Gaussian each way.  After gigs_ctx_set_split_sh(ctx, sh_rest), gigs_forward(ctx, ...) takes `shs` as the
 * degree-0 tensor and reads coefficients 1..M-1 from sh_rest (M is still the total count): same colours bit for bit, no
 * concatenated copy.  The backward of such a forward is the materials-only one (gigs_ctx_set_materials_only, which does not
 * touch SH); gigs_backward refuses anything else.  sh_rest == NULL restores the single tensor. */
int gigs_ctx_set_split_sh(gigs_ctx* ctx, const float* sh_rest);

/* Optional scheduling hook: a hipEvent_t (caller-owned, NULL = none) that gigs_forward records on its stream right
 * before it launches the alpha-blend kernel, so that a caller can start independent work on another stream next to
 * that kernel (it is latency-bound and leaves most CUs idle) rather than next to the bandwidth-bound binning kernels.
 * Per context: forwards issued with `ctx` record it, others do not. */
int gigs_ctx_set_blend_begin_event(gigs_ctx* ctx, void* hip_event);

/* One-wave kernel that occupies `stream` for about `nanoseconds` (it spins on the constant-rate wall clock; capped at
 * 1 ms; capturable into a hipGraph).  Inside a graph, kernel nodes that become ready together start in an order the
 * caller cannot choose; a short head start for the branch that carries a latency-bound kernel (the blend backward's
 * long tiles) ahead of a branch that floods every CU (the light's GGX backward) is expressed as a delay node at the
 * head of the latter (pipeline.WholeStepGraph).  gigs-hip extension. */
int gigs_stream_delay(unsigned nanoseconds, void* stream);

/* Asynchronous binning (gigs-hip extension).  The reference's forward reads the instance count back in the middle
 * (rasterizer_impl.cu:589-594) to size the binning buffer, which serialises host and device and keeps the forward out
 * of a hipGraph.  After gigs_ctx_set_async_binning(ctx, r_capacity > 0, counters) every gigs_forward(ctx, ...) asks the
 * binning callback for gigs_required_binning(r_capacity) bytes, bins at most r_capacity instances, reads nothing back
 * and RETURNS r_capacity (pass it to gigs_backward as R: both carve the same layout).  `counters` (device, 2 x u32, may
 * be NULL) receives {actual instance count, the count again if it exceeded the capacity else 0}; on overflow the surplus
 * instances are dropped (memory-safe, wrong image): the caller checks the flag when convenient, grows the capacity
 * and repeats the step.  r_capacity = 0 restores the synchronous behaviour.  Needs the tile-bucketed binning path
 * (options.binning_legacy = 0) and <= 16384 tiles.  Per context: two contexts may bin with different capacities and
 * counters on two streams at the same time. */
int gigs_ctx_set_async_binning(gigs_ctx* ctx, int r_capacity, unsigned* device_counters);

/* In-library stage timing for bench.py.  Between gigs_profile_begin() and gigs_profile_end()
 * every kernel stage launched by this library records a hipEvent pair on its own stream (no
 * synchronisation is added).  gigs_profile_end() waits for the recorded events, writes the
 * summed milliseconds and launch counts per stage id into the two arrays of length n and
 * returns the number of stage ids; gigs_profile_stage_name(i) names stage i. */
void gigs_profile_begin(void);
int gigs_profile_end(float* total_ms, int* launches, int n);
const char* gigs_profile_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* GIGS_HIP_H_ */
