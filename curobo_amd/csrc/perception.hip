// perception.hip -- the depth front end of curobo_amd.perception (gfx950, wave64).
//
//   curobo_hip_filter_depth   range check, flying-pixel rejection and bilateral smoothing of (B, H, W) depth images
//                             (reference perception/filter_depth.py + mapper/kernel/wp_filter_depth.py)
//   curobo_hip_robot_mask     depth x rays -> camera pose -> closest robot sphere -> threshold -> masked depth, one launch
//                             (reference perception/robot_segmenter.py: _mask_op / _mask_spheres_image)
//
// Both are per-pixel and memory bound when the sphere count is small: a pixel is read once, every neighbour tap and
// every sphere comes from LDS, and nothing of size pixels x spheres or pixels x taps is ever written.
#include "common.hpp"

namespace curobo_hip {

// ------------------------------------------------------------------------------------------ depth filter
// A workgroup of 256 lanes owns a 64 x 16 tile: lane x = tid % 64 (row-contiguous: loads and stores of a wavefront
// are one 256-byte row segment), rows tid / 64 + 4 k.  The tile plus its halo is staged in LDS once.
//
// Semantics (restated from the reference kernels):
//   range     a pixel is kept when min <= d <= max and d is finite, else depth 0 / valid 0
//   flying    4-neighbours, coordinates clamped into the image (a border pixel is its own neighbour); a neighbour outside
//             [min, max] counts as the centre (NaN is NOT outside: it compares false); rejected when the largest
//             |centre - neighbour| exceeds tolerance * centre, the maximum taken as `a > b ? a : b` pairwise
//             (left, right) (up, down) -- the order decides what a NaN neighbour does
//   bilateral taps inside the image and inside [min, max] only, weight exp(-(di^2 + dj^2) / 2 sigma_s^2) *
//             exp(-(dn - dc)^2 / 2 sigma_d^2), rows outer / columns inner; the centre is kept when the weights sum to <= 1e-8
//             (or to NaN)
//   separable (kernel sizes >= 7) the fused pass without smoothing, then a horizontal and a vertical 1-d bilateral pass;
//             their centre test is the range test WITHOUT the finite test, and the valid mask is that of the first pass.
//             A rejected pixel carries 0 into both 1-d passes; with min <= 0 that 0 is in range there, is smoothed like any
//             other pixel and is a tap of its neighbours (as in the reference), but the image that leaves the last pass holds
//             0 wherever the valid mask does: "rejected pixels are 0" holds for every kernel size
constexpr int kTileW = 64, kTileH = 16, kFilterThreads = 256, kRowsPerLane = kTileH / (kFilterThreads / kTileW);
constexpr int kMaxFilterRadius = 15;

enum : int { FILTER_FUSED = 0, FILTER_ROWS = 1, FILTER_COLS = 2 };

struct FilterArgs {
  const float *in;
  float *out;
  uint8_t *valid;
  int H, W;
  float dmin, dmax;
  int enable_flying;
  float flying_tolerance;
  int enable_bilateral, radius;
  float sigma_spatial_sq2, sigma_depth_sq2;
  int halo_x, halo_y;
};

__device__ __forceinline__ float pick_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ bool out_of_range(float d, float lo, float hi) { return d < lo || d > hi; }

template <int MODE>
__global__ __launch_bounds__(kFilterThreads) void filter_depth_kernel(FilterArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int hx = a.halo_x, hy = a.halo_y;
  const int lw = kTileW + 2 * hx, lh = kTileH + 2 * hy;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const size_t image = (size_t)blockIdx.z * (size_t)a.H * (size_t)a.W;
  const float *in = a.in + image;
  float *spatial = lds + lw * lh;  // (2 r + 1)^2 (fused) or 2 r + 1 (1-d passes) spatial weights

  for (int i = tid; i < lw * lh; i += kFilterThreads) {
    const int ly = i / lw, lx = i - ly * lw;
    const int gy = y0 + ly - hy, gx = x0 + lx - hx;
    float v = 0.0f;  // outside the image: never read as a value (every tap checks its coordinates)
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = in[(size_t)gy * a.W + gx];
    lds[i] = v;
  }
  const int r = a.radius, k = 2 * r + 1;
  if (MODE != FILTER_FUSED || a.enable_bilateral) {
    const int n = MODE == FILTER_FUSED ? k * k : k;
    for (int i = tid; i < n; i += kFilterThreads) {
      const int di = MODE == FILTER_FUSED ? i / k - r : i - r, dj = MODE == FILTER_FUSED ? i % k - r : 0;
      spatial[i] = expf(-(float)(di * di + dj * dj) / a.sigma_spatial_sq2);
    }
  }
  __syncthreads();

  const int tx = tid % kTileW, gx = x0 + tx;
  if (gx >= a.W) return;
#pragma unroll
  for (int rr = 0; rr < kRowsPerLane; rr++) {
    const int ty = tid / kTileW + rr * (kFilterThreads / kTileW), gy = y0 + ty;
    if (gy >= a.H) break;
    const size_t o = image + (size_t)gy * a.W + gx;
    const float *c = lds + (ty + hy) * lw + tx + hx;
    const float dc = *c;
    if (MODE == FILTER_FUSED) {
      if (out_of_range(dc, a.dmin, a.dmax) || !isfinite(dc)) {
        a.out[o] = 0.0f;
        a.valid[o] = 0;
        continue;
      }
      if (a.enable_flying) {
        float dl = gx > 0 ? c[-1] : dc, dr = gx + 1 < a.W ? c[1] : dc;
        float du = gy > 0 ? c[-lw] : dc, dd = gy + 1 < a.H ? c[lw] : dc;
        if (out_of_range(dl, a.dmin, a.dmax)) dl = dc;
        if (out_of_range(dr, a.dmin, a.dmax)) dr = dc;
        if (out_of_range(du, a.dmin, a.dmax)) du = dc;
        if (out_of_range(dd, a.dmin, a.dmax)) dd = dc;
        const float m = pick_max(pick_max(fabsf(dc - dl), fabsf(dc - dr)), pick_max(fabsf(dc - du), fabsf(dc - dd)));
        if (m > a.flying_tolerance * dc) {
          a.out[o] = 0.0f;
          a.valid[o] = 0;
          continue;
        }
      }
      a.valid[o] = 1;
      if (!a.enable_bilateral) {
        a.out[o] = dc;
        continue;
      }
    } else if (out_of_range(dc, a.dmin, a.dmax) || (MODE == FILTER_COLS && !a.valid[o])) {
      a.out[o] = 0.0f;
      continue;
    }
    float sum_val = 0.0f, sum_weight = 0.0f;
    const int ri = MODE == FILTER_ROWS ? 0 : r, rj = MODE == FILTER_COLS ? 0 : r;
    for (int di = -ri; di <= ri; di++) {
      if (gy + di < 0 || gy + di >= a.H) continue;
      for (int dj = -rj; dj <= rj; dj++) {
        if (gx + dj < 0 || gx + dj >= a.W) continue;
        const float dn = c[di * lw + dj];
        if (out_of_range(dn, a.dmin, a.dmax)) continue;
        const float ws = spatial[MODE == FILTER_FUSED ? (di + r) * k + dj + r : di + dj + r];
        const float diff = dn - dc;
        const float w = ws * expf(-(diff * diff) / a.sigma_depth_sq2);
        sum_val += dn * w;
        sum_weight += w;
      }
    }
    a.out[o] = sum_weight > 1e-8f ? sum_val / sum_weight : dc;
  }
}

template <int MODE>
static void launch_filter(FilterArgs a, int B, hipStream_t st) {
  const int r = a.radius, k = 2 * r + 1;
  if (MODE == FILTER_FUSED) {
    a.halo_x = a.halo_y = a.enable_bilateral ? (r > 1 ? r : 1) : (a.enable_flying ? 1 : 0);
  } else {
    a.halo_x = MODE == FILTER_ROWS ? r : 0;
    a.halo_y = MODE == FILTER_COLS ? r : 0;
  }
  const size_t lds = sizeof(float) * ((size_t)(kTileW + 2 * a.halo_x) * (kTileH + 2 * a.halo_y) + (size_t)k * k);
  const dim3 grid((unsigned)ceil_div(a.W, kTileW), (unsigned)ceil_div(a.H, kTileH), (unsigned)B);
  hipLaunchKernelGGL(filter_depth_kernel<MODE>, grid, dim3(kFilterThreads), lds, st, a);
}

// ------------------------------------------------------------------------------------------ robot mask
// A pixel is masked when depth > 0 and some enabled sphere (radius >= 0) has r - |p - c| > -threshold, p the pixel's point
// in the robot frame.  Tested without a square root per sphere as |p - c|^2 < (r + threshold)^2 with r + threshold > 0:
// the two forms differ by fp32 rounding of metre-sized numbers (~1e-7 m).  The workgroup turns the spheres into
// (c, (r + threshold)^2 or -1) in LDS once; every lane then holds kMaskPixels pixels in registers and walks the table,
// one broadcast 16-byte LDS read per sphere for 4 x 7 vector instructions.
constexpr int kMaskThreads = 256, kMaskPixels = 4, kMaskChunk = 2048;  // 32 KiB of spheres per pass

__device__ __forceinline__ float round_bf16(float x) {  // fp32 -> bf16 (nearest even) -> fp32; NaN stays NaN
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return x;
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  return __builtin_bit_cast(float, u);
}

struct MaskArgs {
  const float *depth, *rays, *cam_position, *cam_quaternion, *spheres;
  uint8_t *mask;
  float *depth_out;
  int n_pixels, n_spheres;
  int ray_batched, pose_batched, sphere_batched;
  float threshold;
  int bf16_ops;
};

__global__ __launch_bounds__(kMaskThreads) void robot_mask_kernel(MaskArgs a) {
  __shared__ float4 table[kMaskChunk];
  const int tid = threadIdx.x, b = blockIdx.y;
  const size_t image = (size_t)b * a.n_pixels;
  const float *rays = a.rays + (a.ray_batched ? image * 3 : 0);
  const float *pos = a.cam_position + (a.pose_batched ? b * 3 : 0);
  const float *quat = a.cam_quaternion + (a.pose_batched ? b * 4 : 0);
  const float4 *spheres = reinterpret_cast<const float4 *>(a.spheres) + (a.sphere_batched ? (size_t)b * a.n_spheres : 0);
  const float qw = quat[0], qx = quat[1], qy = quat[2], qz = quat[3];
  const float px = pos[0], py = pos[1], pz = pos[2];
  const int base = blockIdx.x * (kMaskThreads * kMaskPixels);

  float d[kMaskPixels], x[kMaskPixels], y[kMaskPixels], z[kMaskPixels];
  bool hit[kMaskPixels];
#pragma unroll
  for (int k = 0; k < kMaskPixels; k++) {
    const int i = min(base + k * kMaskThreads + tid, a.n_pixels - 1);  // lanes past the end repeat the last pixel and store nothing
    d[k] = a.depth[image + i];
    float dd = d[k], rx = rays[3 * (size_t)i], ry = rays[3 * (size_t)i + 1], rz = rays[3 * (size_t)i + 2];
    float cx, cy, cz;
    if (a.bf16_ops) {
      dd = round_bf16(dd);
      cx = round_bf16(dd * round_bf16(rx)), cy = round_bf16(dd * round_bf16(ry)), cz = round_bf16(dd * round_bf16(rz));
    } else {
      cx = dd * rx, cy = dd * ry, cz = dd * rz;
    }
    // p = position + q v q*: v (2 w^2 - 1) + 2 w (u x v) + 2 u (u . v), u = (qx, qy, qz)
    const float s = 2.0f * qw * qw - 1.0f, w2 = 2.0f * qw, ud = 2.0f * (qx * cx + qy * cy + qz * cz);
    x[k] = cx * s + (qy * cz - qz * cy) * w2 + qx * ud + px;
    y[k] = cy * s + (qz * cx - qx * cz) * w2 + qy * ud + py;
    z[k] = cz * s + (qx * cy - qy * cx) * w2 + qz * ud + pz;
    hit[k] = false;
  }
  for (int s0 = 0; s0 < a.n_spheres; s0 += kMaskChunk) {
    const int n = min(kMaskChunk, a.n_spheres - s0);
    if (s0) __syncthreads();
    for (int i = tid; i < n; i += kMaskThreads) {
      float4 s = spheres[s0 + i];
      if (a.bf16_ops) s = make_float4(round_bf16(s.x), round_bf16(s.y), round_bf16(s.z), round_bf16(s.w));
      const float reach = s.w + a.threshold;
      s.w = (s.w >= 0.0f && reach > 0.0f) ? reach * reach : -1.0f;  // a disabled sphere (negative radius) never masks
      table[i] = s;
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {
      const float4 s = table[i];
#pragma unroll
      for (int k = 0; k < kMaskPixels; k++) {
        const float dx = x[k] - s.x, dy = y[k] - s.y, dz = z[k] - s.z;
        hit[k] |= dx * dx + dy * dy + dz * dz < s.w;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMaskPixels; k++) {
    const int i = base + k * kMaskThreads + tid;
    if (i >= a.n_pixels) continue;
    const bool m = d[k] > 0.0f && hit[k];
    a.mask[image + i] = m ? 1 : 0;
    a.depth_out[image + i] = m ? 0.0f : d[k];
  }
}

}  // namespace curobo_hip

using namespace curobo_hip;

CUROBO_EXPORT int curobo_hip_filter_depth(float *depth_out, uint8_t *valid_mask_out, const float *depth_in, float *temp_a,
                                          float *temp_b, int batch, int height, int width, float depth_minimum_distance,
                                          float depth_maximum_distance, int enable_flying_pixel, float flying_tolerance,
                                          int bilateral_kernel_size, float sigma_spatial_sq2, float sigma_depth_sq2,
                                          curobo_hip_stream_t stream) {
  const char *what = "filter_depth";
  CUROBO_REQUIRE(batch >= 0 && height >= 1 && width >= 1, "%s: depth must be (B, H, W) with H, W >= 1, got (%d, %d, %d)", what,
                 batch, height, width);
  CUROBO_REQUIRE(batch <= 65535, "%s: at most 65535 images per launch, got %d", what, batch);
  CUROBO_REQUIRE(bilateral_kernel_size >= 0, "%s: bilateral_kernel_size must be odd (0 disables it), got %d", what,
                 bilateral_kernel_size);
  CUROBO_REQUIRE(bilateral_kernel_size == 0 || bilateral_kernel_size % 2 == 1, "%s: bilateral_kernel_size must be odd, got %d", what,
                 bilateral_kernel_size);
  CUROBO_REQUIRE(bilateral_kernel_size <= 2 * kMaxFilterRadius + 1, "%s: bilateral_kernel_size is at most %d, got %d", what,
                 2 * kMaxFilterRadius + 1, bilateral_kernel_size);
  CUROBO_REQUIRE(depth_in && depth_out && valid_mask_out, "%s: depth_in, depth_out and valid_mask_out must not be null", what);
  CUROBO_REQUIRE(depth_in != depth_out, "%s: depth_out must not alias depth_in (neighbours are read after the centre is written)", what);
  const bool separable = bilateral_kernel_size >= 7;
  CUROBO_REQUIRE(!separable || (temp_a && temp_b && temp_a != temp_b && temp_b != depth_out && temp_a != depth_in),
                 "%s: kernel sizes >= 7 run as three passes and need two distinct (B, H, W) scratch images", what);
  CUROBO_REQUIRE(bilateral_kernel_size == 0 || (sigma_spatial_sq2 > 0.0f && sigma_depth_sq2 > 0.0f),
                 "%s: 2 sigma^2 of the bilateral weights must be positive", what);
  if (batch == 0) return CUROBO_HIP_OK;
  hipStream_t st = (hipStream_t)stream;
  FilterArgs a{};
  a.in = depth_in, a.out = separable ? temp_a : depth_out, a.valid = valid_mask_out;
  a.H = height, a.W = width, a.dmin = depth_minimum_distance, a.dmax = depth_maximum_distance;
  a.enable_flying = enable_flying_pixel != 0, a.flying_tolerance = flying_tolerance;
  a.enable_bilateral = bilateral_kernel_size > 0 && !separable;
  a.radius = a.enable_bilateral ? bilateral_kernel_size / 2 : 0;
  a.sigma_spatial_sq2 = sigma_spatial_sq2, a.sigma_depth_sq2 = sigma_depth_sq2;
  launch_filter<FILTER_FUSED>(a, batch, st);
  if (separable) {
    a.radius = bilateral_kernel_size / 2;
    a.in = temp_a, a.out = temp_b;
    launch_filter<FILTER_ROWS>(a, batch, st);
    a.in = temp_b, a.out = depth_out;
    launch_filter<FILTER_COLS>(a, batch, st);
  }
  return check_launch(what, st);
}

CUROBO_EXPORT int curobo_hip_robot_mask(uint8_t *mask_out, float *depth_out, const float *depth, const float *projection_rays,
                                        const float *camera_position, const float *camera_quaternion, const float *robot_spheres,
                                        int batch, int height, int width, int num_spheres, int ray_batch, int pose_batch,
                                        int sphere_batch, float distance_threshold, int bf16_ops, curobo_hip_stream_t stream) {
  const char *what = "robot_mask";
  CUROBO_REQUIRE(batch >= 0 && height >= 1 && width >= 1, "%s: depth must be (B, H, W) with H, W >= 1, got (%d, %d, %d)", what,
                 batch, height, width);
  CUROBO_REQUIRE(batch <= 65535, "%s: at most 65535 images per launch, got %d", what, batch);
  CUROBO_REQUIRE((int64_t)height * width <= (int64_t)1 << 28, "%s: image of %d x %d pixels is too large", what, height, width);
  CUROBO_REQUIRE(num_spheres >= 0, "%s: num_spheres must be >= 0, got %d", what, num_spheres);
  CUROBO_REQUIRE(ray_batch == 1 || ray_batch == batch, "%s: projection rays batch must be 1 or match depth batch: got %d vs %d", what,
                 ray_batch, batch);
  CUROBO_REQUIRE(pose_batch == 1 || pose_batch == batch, "%s: camera pose batch must be 1 or match depth batch: got %d vs %d", what,
                 pose_batch, batch);
  CUROBO_REQUIRE(sphere_batch == 1 || sphere_batch == batch, "%s: robot_spheres batch must be 1 or match points batch: got %d vs %d",
                 what, sphere_batch, batch);
  CUROBO_REQUIRE(bf16_ops == 0 || bf16_ops == 1, "%s: arithmetic mode must be 0 (fp32) or 1 (bf16 ops), got %d", what, bf16_ops);
  CUROBO_REQUIRE(mask_out && depth_out && depth && projection_rays && camera_position && camera_quaternion,
                 "%s: mask_out, depth_out, depth, projection_rays, camera_position and camera_quaternion must not be null", what);
  CUROBO_REQUIRE(robot_spheres || num_spheres == 0, "%s: robot_spheres must not be null", what);
  CUROBO_REQUIRE(((uintptr_t)robot_spheres & 15) == 0, "%s: robot_spheres must be 16-byte aligned", what);
  if (batch == 0) return CUROBO_HIP_OK;
  hipStream_t st = (hipStream_t)stream;
  MaskArgs a{};
  a.depth = depth, a.rays = projection_rays, a.cam_position = camera_position, a.cam_quaternion = camera_quaternion;
  a.spheres = robot_spheres, a.mask = mask_out, a.depth_out = depth_out;
  a.n_pixels = height * width, a.n_spheres = num_spheres;
  a.ray_batched = ray_batch != 1, a.pose_batched = pose_batch != 1, a.sphere_batched = sphere_batch != 1;
  a.threshold = distance_threshold, a.bf16_ops = bf16_ops;
  const dim3 grid((unsigned)ceil_div(a.n_pixels, kMaskThreads * kMaskPixels), (unsigned)batch);
  hipLaunchKernelGGL(robot_mask_kernel, grid, dim3(kMaskThreads), 0, st, a);
  return check_launch(what, st);
}
