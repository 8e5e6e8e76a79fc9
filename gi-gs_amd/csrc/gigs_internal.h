// gigs_internal.h -- what the library's translation units share on the HOST side and nobody outside sees: the
// profile stage ids, the stack-scoped stage timer, the error helper, the options accessor, the launch check and the
// ray table of the screen-space marches.  Not installed; everything declared here has hidden visibility and is
// defined in api.hip, but for the ray table (gi.hip).
#pragma once
#include "../../include/gigs_hip.h"
#include "gigs_common.h"

#define GIGS_HIDDEN __attribute__((visibility("hidden")))

namespace gigs {

// ---- profile stages (gigs_profile_end / gigs_profile_stage_name) ------------------------------------------------
// Tools key on the NAMES; the numbers index the caller's arrays.  A new stage goes in front of kCount here and at the
// end of kStageNames -- nowhere else.
enum class Stage : int {
  kPreprocess = 0, kScan, kDuplicate, kSort, kRanges, kBlendFwd, kBlendBwd, kPreprocessBwd,
  kDepthToNormal, kSsao, kSsr, kMedian, kBilateral, kMedianBwd, kShadeFwd, kShadeBwd,
  kCubemapFwd, kCubemapBwd, kGbufferPost, kLossFwd, kLossBwd, kL1SsimFwd, kL1SsimBwd, kTvFwd, kTvBwd,
  kMaskedL1, kAdam, kDensifyStats, kGatherRows, kDist2, kActivateFwd, kActivateBwd, kCount
};
constexpr const char* kStageNames[] = {
  "preprocess_fwd", "scan", "duplicate", "sort", "tile_ranges", "blend_fwd", "blend_bwd",
  "preprocess_bwd", "depth_to_normal", "ssao", "ssr", "median3x3", "bilateral3x3",
  "median3x3_bwd", "shade_fwd", "shade_bwd", "cubemap_fwd", "cubemap_bwd", "gbuffer_post",
  "stage2_loss_fwd", "stage2_loss_bwd", "l1_ssim_fwd", "l1_ssim_bwd", "tv_loss_fwd", "tv_loss_bwd", "masked_l1",
  "adam_step", "densify_stats", "gather_rows", "dist2", "activate_fwd", "activate_bwd"};
static_assert(sizeof(kStageNames) / sizeof(kStageNames[0]) == (size_t)Stage::kCount, "one name per stage");

// Times what is launched on `stream` during its lifetime as one launch of `stage` when a profile session is active
// (an event pair, no synchronisation); otherwise it costs one relaxed atomic load.  Leaves with the scope, so an
// early return cannot lose it.
class GIGS_HIDDEN StageTimer {
 public:
  StageTimer(Stage stage, void* stream);  // stream: a hipStream_t
  ~StageTimer();
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;

 private:
  hipStream_t s_;
  Stage stage_;
  bool on_;
  hipEvent_t a_, b_;
};

// ---- the ray set of SSAO / SSR -----------------------------------------------------------------------------------
// One table per (device, delta) and process, built on first use and never modified; gi.hip owns the cache and
// describes the layout.  `out` is a copy of the entry; 0, or -1 for an unusable delta, -2 for a HIP failure.
struct RayTable {
  int device = -1;
  float delta = -1.0f;
  int nrays = 0;   // all rays of the reference's loops (SSR's nrSamples)
  int n_live = 0;  // rays with a non-zero weight: table entries [0, n_live)
  int n_dead = 0;  // identical zero-weight rays: entries [n_live, n_live + n_dead)
  float sum_w = 0.0f;  // SSAO's nrSamples, accumulated in fp32 in ray order
  float4* dev = nullptr;
};
GIGS_HIDDEN int get_ray_table(float delta, hipStream_t s, RayTable& out);

}  // namespace gigs

extern "C" {
// the context's options (NULL = the defaults)
GIGS_HIDDEN const gigs::Options* gigs_internal_options(const gigs_ctx* ctx);
// records `msg` for gigs_last_error() and returns `code`
GIGS_HIDDEN int gigs_internal_fail(int code, const char* msg);
// after the launches of an entry point: 0, or GIGS_ERR_HIP with "<entry>: launch failed: <hipGetErrorString>" recorded
GIGS_HIDDEN int gigs_internal_check_launch(const char* entry);
}
