// Occupancy grids for scenes (include/aon_hip_scene_occ.h is the contract, tests/_scene_occ_ref.py the yardstick):
// the stage call that runs aon_occ.hip's mark / scan / emit on the K object segments of a scene's pair rows at once, each segment against
// its own object's grid, and then the GATHER instance of art_mlp_fwd_kernel per object.  Three compaction launches per level whatever K is,
// no atomics: the same bits on every run.
//
// A pair's ray is already in its object's frame, so a grid built in that frame applies verbatim: x = o' + t d' (multiply, then add: the MLP
// kernel's own bits), looked up by occ_lookup (aon_occ_lookup.h).  Object k has ceil(P_k S / 1024) tiles when it has a grid and none
// otherwise (a DENSE segment: not touched, its counter all of its samples); its list holds SEGMENT-LOCAL sample indices row_local * S + i at
// idx + starts[k] S, so each segment feeds the GATHER launch unchanged with its own ray / t / raw pointers.
#include "../../include/aon_hip_scene_occ.h"
#include "aon_capi_util.h"

using namespace aon::capi;

extern "C" {

int64_t aon_scene_occ_workspace_bytes(int64_t pairs, int k, int s) {
  if (pairs < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 1 || pairs > (int64_t)0x7fffffff / s) return 0;
  return aon::scene_occ_list_bytes(pairs, k, s);
}

int aon_scene_art_mlp_fwd_occ(const void* packed, const void* const* smalls_host, const aon_occupancy* const* grids_host, const int64_t* starts_host,
                              const float* pair_o, const float* pair_d, const float* pair_v, const float* t_vals, int k, int s, float* raw,
                              int64_t* occupied_dev, void* workspace, int64_t workspace_bytes, void* stream_) {
  auto bad = [&](const std::string& what) { return fail(AON_E_INVALID, ("aon_scene_art_mlp_fwd_occ: " + what).c_str()); };
  if (k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 1) return bad("bad object count / sample count (1 <= k <= 16, s >= 1)");
  bool ascending = starts_host && starts_host[0] == 0;
  for (int j = 0; ascending && j < k; ++j) ascending = starts_host[j + 1] >= starts_host[j];
  if (!ascending) return bad("starts_host must ascend from starts_host[0] = 0");
  const int64_t pairs = starts_host[k];
  if (pairs > (int64_t)0x7fffffff / s) return bad("more than 2^31 - 1 samples (starts_host[k] * s)");
  if (pairs == 0) return AON_OK;
  bool null = !packed || !smalls_host || !grids_host || !pair_o || !pair_d || !pair_v || !t_vals || !raw || !workspace;
  for (int j = 0; !null && j < k; ++j) null = starts_host[j + 1] > starts_host[j] && !smalls_host[j];
  if (null) return bad("null pointer");
  aon::OccGrid grids[AON_SCENE_MAX_OBJECTS];
  std::memset(grids, 0, sizeof(grids));
  for (int j = 0; j < k; ++j)
    if (grids_host[j])
      if (const char* msg = occ_grid_bad(grids_host[j], grids[j])) return bad("object " + std::to_string(j) + ": " + msg);
  if ((reinterpret_cast<uintptr_t>(raw) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255))
    return bad("raw must be 16-byte aligned and the workspace 256-byte aligned");
  for (int j = 0; j < k; ++j)
    if (starts_host[j + 1] > starts_host[j] && forms_differ(packed, smalls_host[j])) return fail(AON_E_INVALID, kFormsMsg);
  if (workspace_bytes < aon_scene_occ_workspace_bytes(pairs, k, s))
    return fail(AON_E_WORKSPACE, "aon_scene_art_mlp_fwd_occ: workspace smaller than aon_scene_occ_workspace_bytes()");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int* idx = nullptr;
  const int64_t* counts = nullptr;
  const aon::OccCompact compact{grids, starts_host, k, s, 0, s, pair_o, pair_d, t_vals, nullptr, nullptr};
  if (int rc = check(aon::launch_occ_compact(compact, raw, static_cast<char*>(workspace), aon::scene_occ_tile_cap(pairs, k, s), occupied_dev, &idx, &counts,
                                             stream), "aon_scene_art_mlp_fwd_occ (compact)"))
    return rc;
  // one MLP launch per object with rows, as aon_art_mlp_fwd makes it (no per-ray view bias): on the object's list, or dense
  for (int j = 0; j < k; ++j) {
    const int64_t r0 = starts_host[j], rows = starts_host[j + 1] - r0;
    if (rows == 0) continue;
    MlpTimer timer(stream, rows * s);
    aon::FwdSeg seg{.packed = static_cast<const char*>(packed), .small = static_cast<const float*>(smalls_host[j]), .rays_o = pair_o + r0 * 3,
                    .rays_d = pair_d + r0 * 3, .viewdirs = pair_v + r0 * 3, .t_vals = t_vals + r0 * s, .n_rays = rows, .S = s, .raw = raw + r0 * s * 4};
    if (grids[j].bits) { seg.gather_idx = idx + r0 * s; seg.gather_count = counts + j; seg.max_listed = rows * s; }
    if (int rc = check(aon::launch_net_fwd(true, &seg, 1, stream), "aon_scene_art_mlp_fwd_occ")) return rc;
  }
  return AON_OK;
}

}  // extern "C"
