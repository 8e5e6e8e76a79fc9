// mesh_clean.hip -- cleaning an extracted mesh: connected components of the faces, a keep decision per component, and
// the compaction of what is kept.  include/gigs_hip.h states every quantity; all of them are integers that do not
// depend on the order of execution, and tests/mesh_clean_ref.py restates them in numpy.
//
// The labelling is a parent forest over the vertices with min-hooking:
//   invariant   0 <= parent[x] <= x for every x.  The caller initialises parent[x] = x; hook_kernel lowers entries with
//               atomicMin only and flatten_kernel replaces parent[v] by a vertex further down v's own chain, so the
//               invariant holds at every instant, whatever the interleaving.
//   walking     root_of() follows x <- parent[x] while parent[x] < x.  Every step strictly decreases x, so the walk ends
//               after at most x steps WITHOUT REFERENCE TO ANY OTHER THREAD'S PROGRESS.  It is the only device loop in
//               this file: there is no compare-and-swap retry, no spin, no ticket and no wait anywhere, and a value
//               outside [0, x) ends the walk, so no content of `parent` can make a thread loop or read out of bounds.
//   hook_kernel one thread per valid face: the three roots by walking, m = their minimum, and atomicMin(parent[r], m)
//               for every root r > m; *changed = 1 if the roots differed.
//   staleness   A thread acts on what it read: r may have stopped being a root by the time its atomicMin lands (another
//               face hooked r under k in between, or the read came from a cache line older than that hook).  The
//               atomicMin then leaves parent[r] = min(k, m), and if m < k the link r -> k is gone: the forest of this
//               instant may no longer join r's tree with k's.  Nothing is wrong yet, because (a) every value ever
//               stored into parent[r] is a vertex that a chain of valid faces joins to r, so a tree never spans two
//               components, and (b) the face that asked for r -> k is examined again by the next pass, finds two
//               different roots and hooks again.  The result is taken only from a pass that leaves *changed == 0: such a
//               pass performed no store at all, so every one of its threads read the same, static forest and found its
//               three vertices under one root.  Trees within components (a) + every face within one tree = the trees
//               are the components; and since parent[x] <= x along every chain, each root is its tree's smallest
//               index.  The host alternates hook and flatten until that confirming pass, so `parent` is then the flat
//               label array (flatten ran last, or nothing was ever hooked and parent is still the identity).
//   progress    A pass that sets *changed lowers the parent of at least one vertex that was a root, so the number of
//               roots falls: at most V passes in any schedule.  The host's cap is far lower (mesh.py, DESIGN.md
//               "Cleaning meshes") and reaching it is an error, never a result.
#include "mesh_grid.h"  // item, in_range, blocks_for

namespace gigs {
namespace mesh_clean {

using namespace gigs::mesh_common;

// the root of x's chain.  Ends by itself: x strictly decreases; p outside [0, x) (a root, or corrupt input) stops it.
__device__ __forceinline__ int root_of(const int* parent, int x) {
  for (;;) {
    const int p = parent[x];
    if (p < 0 || p >= x) return x;
    x = p;
  }
}

__global__ __launch_bounds__(256) void hook_kernel(int V, int F, const int* __restrict__ faces, int* parent, int* changed) {
  const int f = item<256>(F);
  if (f < 0) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  if (!in_range(a, b, c, V)) return;  // never dereferenced
  const int ra = root_of(parent, a), rb = root_of(parent, b), rc = root_of(parent, c);
  const int m = min(ra, min(rb, rc));
  if (ra == m && rb == m && rc == m) return;
  if (ra != m) atomicMin(parent + ra, m);
  if (rb != m) atomicMin(parent + rb, m);
  if (rc != m) atomicMin(parent + rc, m);
  *changed = 1;  // plain stores of the same value
}

__global__ __launch_bounds__(256) void flatten_kernel(int V, int* parent) {
  const int v = item<256>(V);
  if (v < 0) return;
  // no root changes during this kernel and every concurrent store replaces an entry by a vertex further down the same
  // chain, so the walk reaches v's root whichever of the two values it reads
  const int r = root_of(parent, v);
  if (r != v) parent[v] = r;
}

// face_label, count per root and the number of invalid faces.  `parent` is flat.  A wave first agrees on the label of
// its first valid lane: the lanes that share it (all of them, in a mesh of one large component) send one atomic with
// their number, the others one atomic each.
__global__ __launch_bounds__(256) void count_kernel(int V, int F, const int* __restrict__ faces, const int* __restrict__ parent,
                                                    int* __restrict__ face_label, int* count, int* invalid) {
  const int f = item<256>(F);
  int label = -2;  // -2: no face, -1: an invalid face
  if (f >= 0) {
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    label = -1;
    if (in_range(a, b, c, V)) {
      const int r = parent[a];
      label = (r >= 0 && r < V) ? r : -1;  // a flat parent array never takes the second branch
    }
    face_label[f] = label;
  }
  const int lane = (int)__lane_id();
  const unsigned long long bad = __ballot(label == -1);
  const unsigned long long good = __ballot(label >= 0);
  if (bad != 0 && lane == __ffsll((long long)bad) - 1) atomicAdd(invalid, __popcll(bad));
  if (good != 0) {  // wave-uniform
    const int leader = __ffsll((long long)good) - 1;
    const int lead = __shfl(label, leader);
    const unsigned long long same = __ballot(label == lead);
    if (label == lead) {
      if (lane == leader) atomicAdd(count + lead, __popcll(same));
    } else if (label >= 0) {
      atomicAdd(count + label, 1);
    }
  }
}

__global__ __launch_bounds__(256) void mark_kernel(int V, int F, const int* __restrict__ faces, const int* __restrict__ face_label,
                                                   const uint8_t* __restrict__ root_keep, int* __restrict__ face_keep,
                                                   int* vertex_keep) {
  const int f = item<256>(F);
  if (f < 0) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  const int r = face_label[f];
  const bool keep = in_range(a, b, c, V) && r >= 0 && r < V && root_keep[r] != 0;
  face_keep[f] = keep ? 1 : 0;
  if (keep) {
    vertex_keep[a] = 1;  // plain stores of the same value
    vertex_keep[b] = 1;
    vertex_keep[c] = 1;
  }
}

struct MeshIn {
  const float *vertices, *normals, *albedo, *roughness, *metallic;
};
struct MeshOut {
  float *vertices, *normals, *albedo, *roughness, *metallic;
};

__global__ __launch_bounds__(256) void compact_vertices_kernel(int V, MeshIn in, const int* __restrict__ vertex_keep,
                                                               const int* __restrict__ vertex_offsets, int capacity, MeshOut out,
                                                               int* overflow) {
  const int v = item<256>(V);
  if (v < 0 || vertex_keep[v] == 0) return;
  const int o = vertex_offsets[v];
  if (o < 0 || o >= capacity) {
    *overflow = 1;
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    out.vertices[3 * (size_t)o + c] = in.vertices[3 * (size_t)v + c];
    out.normals[3 * (size_t)o + c] = in.normals[3 * (size_t)v + c];
    out.albedo[3 * (size_t)o + c] = in.albedo[3 * (size_t)v + c];
  }
  out.roughness[o] = in.roughness[v];
  out.metallic[o] = in.metallic[v];
}

__global__ __launch_bounds__(256) void compact_faces_kernel(int V, int F, const int* __restrict__ faces,
                                                            const int* __restrict__ vertex_keep,
                                                            const int* __restrict__ vertex_offsets,
                                                            const int* __restrict__ face_keep,
                                                            const int* __restrict__ face_offsets, int vertex_capacity,
                                                            int face_capacity, int* __restrict__ out_faces, int* overflow) {
  const int f = item<256>(F);
  if (f < 0 || face_keep[f] == 0) return;
  const int o = face_offsets[f];
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  if (o < 0 || o >= face_capacity || !in_range(a, b, c, V)) {
    *overflow = 1;
    return;
  }
  const int na = vertex_offsets[a], nb = vertex_offsets[b], nc = vertex_offsets[c];
  if (vertex_keep[a] == 0 || vertex_keep[b] == 0 || vertex_keep[c] == 0 || !in_range(na, nb, nc, vertex_capacity)) {
    *overflow = 1;  // a kept face on a vertex that was not kept, or a new index outside the vertex outputs
    return;
  }
  out_faces[3 * (size_t)o] = na;
  out_faces[3 * (size_t)o + 1] = nb;
  out_faces[3 * (size_t)o + 2] = nc;
}

}  // namespace mesh_clean
}  // namespace gigs

extern "C" {

int gigs_mesh_cc_hook(int n_vertices, int n_faces, const int* faces, int* parent, int* changed, void* stream) {
  using namespace gigs::mesh_clean;
  if (n_vertices < 0 || n_faces < 0 || !changed || (n_faces > 0 && !faces) || (n_vertices > 0 && !parent))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cc_hook: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(changed, 0, sizeof(int), s) != hipSuccess) return gigs_internal_fail(GIGS_ERR_HIP, "mesh_cc_hook: clear failed");
  if (n_faces == 0 || n_vertices == 0) return 0;
  hipLaunchKernelGGL(hook_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, s, n_vertices, n_faces, faces, parent, changed);
  return gigs_internal_check_launch("mesh_cc_hook");
}

int gigs_mesh_cc_flatten(int n_vertices, int* parent, void* stream) {
  using namespace gigs::mesh_clean;
  if (n_vertices < 0 || (n_vertices > 0 && !parent)) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cc_flatten: bad argument");
  if (n_vertices == 0) return 0;
  hipLaunchKernelGGL(flatten_kernel, dim3(blocks_for(n_vertices)), dim3(256), 0, (hipStream_t)stream, n_vertices, parent);
  return gigs_internal_check_launch("mesh_cc_flatten");
}

int gigs_mesh_cc_count(int n_vertices, int n_faces, const int* faces, const int* parent, int* face_label, int* count,
                       int* invalid_faces, void* stream) {
  using namespace gigs::mesh_clean;
  if (n_vertices < 0 || n_faces < 0 || !invalid_faces || (n_faces > 0 && (!faces || !face_label)) ||
      (n_vertices > 0 && (!parent || !count)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cc_count: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(invalid_faces, 0, sizeof(int), s) != hipSuccess ||
      (n_vertices > 0 && hipMemsetAsync(count, 0, sizeof(int) * (size_t)n_vertices, s) != hipSuccess))
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_cc_count: clear failed");
  if (n_faces == 0) return 0;
  hipLaunchKernelGGL(count_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, s, n_vertices, n_faces, faces, parent, face_label,
                     count, invalid_faces);
  return gigs_internal_check_launch("mesh_cc_count");
}

int gigs_mesh_mark(int n_vertices, int n_faces, const int* faces, const int* face_label, const uint8_t* root_keep,
                   int* face_keep, int* vertex_keep, void* stream) {
  using namespace gigs::mesh_clean;
  if (n_vertices < 0 || n_faces < 0 || (n_faces > 0 && (!faces || !face_label || !face_keep)) ||
      (n_vertices > 0 && (!root_keep || !vertex_keep)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_mark: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (n_vertices > 0 && hipMemsetAsync(vertex_keep, 0, sizeof(int) * (size_t)n_vertices, s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_mark: clear failed");
  if (n_faces == 0) return 0;
  hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, s, n_vertices, n_faces, faces, face_label, root_keep,
                     face_keep, vertex_keep);
  return gigs_internal_check_launch("mesh_mark");
}

int gigs_mesh_compact(int n_vertices, int n_faces, const float* vertices, const float* normals, const float* albedo,
                      const float* roughness, const float* metallic, const int* faces, const int* vertex_keep,
                      const int* vertex_offsets, const int* face_keep, const int* face_offsets, int vertex_capacity,
                      int face_capacity, float* out_vertices, float* out_normals, float* out_albedo, float* out_roughness,
                      float* out_metallic, int* out_faces, int* overflow, void* stream) {
  using namespace gigs::mesh_clean;
  if (n_vertices < 0 || n_faces < 0 || vertex_capacity < 0 || face_capacity < 0 || !overflow)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_compact: bad argument");
  if (n_vertices > 0 && (!vertices || !normals || !albedo || !roughness || !metallic || !vertex_keep || !vertex_offsets))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_compact: NULL vertex input");
  if (n_faces > 0 && (!faces || !face_keep || !face_offsets)) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_compact: NULL face input");
  if (vertex_capacity > 0 && (!out_vertices || !out_normals || !out_albedo || !out_roughness || !out_metallic))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_compact: NULL vertex output");
  if (face_capacity > 0 && !out_faces) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_compact: NULL face output");
  hipStream_t s = (hipStream_t)stream;
  const MeshIn in = {vertices, normals, albedo, roughness, metallic};
  const MeshOut out = {out_vertices, out_normals, out_albedo, out_roughness, out_metallic};
  if (n_vertices > 0)
    hipLaunchKernelGGL(compact_vertices_kernel, dim3(blocks_for(n_vertices)), dim3(256), 0, s, n_vertices, in, vertex_keep,
                       vertex_offsets, vertex_capacity, out, overflow);
  if (n_faces > 0 && n_vertices > 0)
    hipLaunchKernelGGL(compact_faces_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, s, n_vertices, n_faces, faces, vertex_keep,
                       vertex_offsets, face_keep, face_offsets, vertex_capacity, face_capacity, out_faces, overflow);
  return gigs_internal_check_launch("mesh_compact");
}
}  // extern "C"
