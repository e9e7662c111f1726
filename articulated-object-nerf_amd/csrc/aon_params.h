// The parameter layout of the two networks, stated once: where each nn.Linear sits in the `params` / `grads` pointer arrays handed to
// the pack, prepare and backward calls (device pointers to the unmodified torch storages, (out,in) row-major fp32), the row stride of
// every weight whose input is a concatenation, and the column where each block of that concatenation starts.  Constants and constexpr
// functions only.  (include/aon_hip.h describes the same order in prose for the caller.)
#pragma once

namespace aon {

// widths that the layout is made of: trunk, view branch / deformation MLP, and the three latent codes of the articulated network
constexpr int kNetWidth = 256;
constexpr int kCondWidth = 128;
constexpr int kShapeDim = 128, kAppDim = 128, kArtDim = 32;
// columns of a positional encoding with L frequency levels (the input itself, then sin and shifted sin of each level)
__host__ __device__ constexpr int enc_width(int levels) { return 3 + 6 * levels; }

// ---- vanilla NeRFMLP (models/vanilla_nerf/model.py:39-120) ----
//   pts_linears.{0..7}.{weight,bias}, views_linear.0, bottleneck_layer, density_layer, rgb_layer
__host__ __device__ constexpr int vp_trunk_w(int l) { return 2 * l; }
__host__ __device__ constexpr int vp_trunk_b(int l) { return 2 * l + 1; }
constexpr int kVpView0W = 16, kVpView0B = 17;
constexpr int kVpBottW = 18, kVpBottB = 19;
constexpr int kVpSigmaW = 20, kVpSigmaB = 21;
constexpr int kVpRgbW = 22, kVpRgbB = 23;
constexpr int kNumVanillaParams = 24;
// row strides: pts_linears.0 reads enc(P), pts_linears.5 cat[h(256), enc(P)], views_linear.0 cat[bottleneck(256), viewenc(V)]
__host__ __device__ constexpr int vp_trunk0_ld(int P) { return P; }
__host__ __device__ constexpr int vp_trunk5_ld(int P) { return kNetWidth + P; }
__host__ __device__ constexpr int vp_view0_ld(int V) { return kNetWidth + V; }

// ---- articulated NeRFMLP (model_autodecoder.py:60-170) ----
//   deformations_linear.{0..3}, deformation_layer, pts_linears.{0..7}, views_linear.{0..3}, bottleneck_layer, density_layer, rgb_layer
__host__ __device__ constexpr int ap_deform_w(int l) { return 2 * l; }
__host__ __device__ constexpr int ap_deform_b(int l) { return 2 * l + 1; }
constexpr int kApDeformOutW = 8, kApDeformOutB = 9;
__host__ __device__ constexpr int ap_trunk_w(int l) { return 10 + 2 * l; }
__host__ __device__ constexpr int ap_trunk_b(int l) { return 11 + 2 * l; }
__host__ __device__ constexpr int ap_view_w(int l) { return 26 + 2 * l; }
__host__ __device__ constexpr int ap_view_b(int l) { return 27 + 2 * l; }
constexpr int kApBottW = 34, kApBottB = 35;
constexpr int kApSigmaW = 36, kApSigmaB = 37;
constexpr int kApRgbW = 38, kApRgbB = 39;
constexpr int kNumArtParams = 40;
constexpr int kMaxNetParams = kNumArtParams > kNumVanillaParams ? kNumArtParams : kNumVanillaParams;
// row strides and column blocks:
//   deformations_linear.0  cat[pos(3), shape(128), articulation(32)]
//   pts_linears.0          cat[enc(P), shape(128)]
//   pts_linears.5          cat[h(256), enc(P), shape(128)]
//   views_linear.0         cat[bottleneck(256), viewenc(V), appearance(128)]
constexpr int kApDeform0ShapeCol = 3;
constexpr int kApDeform0ArtCol = kApDeform0ShapeCol + kShapeDim;
constexpr int kApDeform0Ld = kApDeform0ArtCol + kArtDim;
__host__ __device__ constexpr int ap_trunk0_shape_col(int P) { return P; }
__host__ __device__ constexpr int ap_trunk0_ld(int P) { return ap_trunk0_shape_col(P) + kShapeDim; }
constexpr int kTrunk5EncCol = kNetWidth;       // (both networks)
__host__ __device__ constexpr int ap_trunk5_shape_col(int P) { return kTrunk5EncCol + P; }
__host__ __device__ constexpr int ap_trunk5_ld(int P) { return ap_trunk5_shape_col(P) + kShapeDim; }
constexpr int kView0EncCol = kNetWidth;        // (both networks)
__host__ __device__ constexpr int ap_view0_app_col(int V) { return kView0EncCol + V; }
__host__ __device__ constexpr int ap_view0_ld(int V) { return ap_view0_app_col(V) + kAppDim; }

// the table tied to itself: the index ranges follow each other without a gap or an overlap, and the last one ends at the count
static_assert(vp_trunk_w(0) == 0 && vp_trunk_b(7) + 1 == kVpView0W && kVpView0B + 1 == kVpBottW && kVpBottB + 1 == kVpSigmaW &&
              kVpSigmaB + 1 == kVpRgbW && kVpRgbB + 1 == kNumVanillaParams, "vanilla parameter order");
static_assert(ap_deform_w(0) == 0 && ap_deform_b(3) + 1 == kApDeformOutW && kApDeformOutB + 1 == ap_trunk_w(0) &&
              ap_trunk_b(7) + 1 == ap_view_w(0) && ap_view_b(3) + 1 == kApBottW && kApBottB + 1 == kApSigmaW &&
              kApSigmaB + 1 == kApRgbW && kApRgbB + 1 == kNumArtParams, "articulated parameter order");
static_assert(vp_trunk_b(0) == vp_trunk_w(0) + 1 && ap_deform_b(0) == ap_deform_w(0) + 1 && ap_trunk_b(0) == ap_trunk_w(0) + 1 &&
              ap_view_b(0) == ap_view_w(0) + 1 && kVpView0B == kVpView0W + 1 && kApBottB == kApBottW + 1, "a bias follows its weight");
// ... and to the shapes the Python side publishes for the default degrees (ops.ART_PARAM_SHAPES, ops.VANILLA_PARAM_SHAPES)
static_assert(enc_width(10) == 63 && enc_width(4) == 27, "default encodings");
static_assert(vp_trunk0_ld(63) == 63 && vp_trunk5_ld(63) == 319 && vp_view0_ld(27) == 283, "vanilla row strides at the default degrees");
static_assert(kApDeform0Ld == 163 && ap_trunk0_ld(63) == 191 && ap_trunk5_ld(63) == 447 && ap_view0_ld(27) == 411,
              "articulated row strides at the default degrees");

// ---- where the latent codes enter the articulated network ----
// Every latent is broadcast to all samples (model_autodecoder.py:186-194), so each entry is a per-call constant of the forward
// (aon_art_prepare folds W[:, col : col + L] . latent into the layer's bias), and of the backward
//   d latent += W[:, col : col + L]^T db        dW[:, col : col + L] = db (x) latent
// with db the layer's bias gradient.  Five entries over four bias gradients (`src`: 0 deformations_linear.0, 1 pts_linears.0,
// 2 pts_linears.5, 3 views_linear.0).  A latent's entries are summed in table order.
enum : int { kLatShape = 0, kLatApp = 1, kLatArt = 2, kNumLatents = 3 };
constexpr int kNumLatentEntries = 5, kNumLatentBiases = 4, kMaxLatentPairs = 3;
struct LatentEntry {
  int latent;     // kLatShape / kLatApp / kLatArt
  int w, b;       // parameter indices of the layer's weight and bias
  int src;        // which of the four bias gradients
  int M;          // rows of the weight
  int ld, col;    // row stride and first column of the latent's block
  int L;          // width of the latent
};
__host__ __device__ constexpr LatentEntry art_latent_entry(int i, int P, int V) {
  return i == 0 ? LatentEntry{kLatShape, ap_deform_w(0), ap_deform_b(0), 0, kCondWidth, kApDeform0Ld, kApDeform0ShapeCol, kShapeDim}
       : i == 1 ? LatentEntry{kLatArt, ap_deform_w(0), ap_deform_b(0), 0, kCondWidth, kApDeform0Ld, kApDeform0ArtCol, kArtDim}
       : i == 2 ? LatentEntry{kLatShape, ap_trunk_w(0), ap_trunk_b(0), 1, kNetWidth, ap_trunk0_ld(P), ap_trunk0_shape_col(P), kShapeDim}
       : i == 3 ? LatentEntry{kLatShape, ap_trunk_w(5), ap_trunk_b(5), 2, kNetWidth, ap_trunk5_ld(P), ap_trunk5_shape_col(P), kShapeDim}
                : LatentEntry{kLatApp, ap_view_w(0), ap_view_b(0), 3, kCondWidth, ap_view0_ld(V), ap_view0_app_col(V), kAppDim};
}
// offset of bias gradient `src` in a packed copy of the four (128 + 256 + 256 + 128 floats)
__host__ __device__ constexpr int lat_db_off(int src) { return src == 0 ? 0 : src == 1 ? 128 : src == 2 ? 384 : 640; }
constexpr int kLatDbFloats = 768;
static_assert(lat_db_off(1) == art_latent_entry(0, 63, 27).M && lat_db_off(2) - lat_db_off(1) == art_latent_entry(2, 63, 27).M &&
              lat_db_off(3) - lat_db_off(2) == art_latent_entry(3, 63, 27).M && kLatDbFloats - lat_db_off(3) == art_latent_entry(4, 63, 27).M,
              "the packed bias gradients follow the table's row counts");

}  // namespace aon
