// Cubemap panoramas, CMP and EAC (the definition is in include/pconv_hip.h, pconv_cube_from_erp_map /
// pconv_cube_pad_f32 / pconv_cube_to_erp_map): the two maps that make a cube conversion a job of the renderer
// (viewport.hip) and the sampler (sphere_sampler.h), and the one kernel the way back needs besides.
//   cube_from_erp_map_kernel  one lane per sample of the (6 a ss) x (a ss) grid of the face stack: its face, its plane
//                             coordinates (through tan for EAC), its direction -- all in fp64 -- and its record on the
//                             h x w ERP source (record_of_direction), one 8-byte store.
//   cube_to_erp_map_kernel    one lane per sample of the (h ss) x (w ss) ERP grid: its direction as in the sphere rotation,
//                             the face it falls on (the tie rule of the header), the position on that face (through atan
//                             for EAC) and the record on the PADDED stack seen as one plane of 6 A x A, A = a + 6.
//   cube_pad_f32_kernel       (n, C, 6 a, a) -> (n, C, 6 A, A): a workgroup takes 4 rows x 64 columns of the padded plane,
//                             a lane one pixel.  An interior pixel is a copy; a ring pixel reads its record (g, qu, qv)
//                             from the host's table and is the bilinear read of face g there, four loads, three lerps.
//                             No trigonometry on the device: the ring is 12 a + 36 pixels per face, the table is built
//                             once per (kind, a) on the host.  One pass, every pixel stored by its own lane.  The depth of
//                             the ring is an argument: 3 for the way back (pconv_cube_pad_f32), 1 .. 8 through
//                             pconv_cube_pad_depth_f32 (A = a + 2 depth; cube.ws_ssim continues by 5, §4k).
//   cube_pad_backward_f32_kernel  the ordered backward of the continuation (pconv_cube_pad_backward_f32): a gather.  A lane owns
//                             one pixel of the face stack, starts from the gradient of its own interior copy and walks
//                             its list of pconv_host_cube_pad_reverse once, front to back, for up to 4 planes at a time
//                             (the decoding of an entry -- its record, its coefficient, its ring pixel -- is shared by
//                             the planes, the sums are not).  Most pixels have no list: only those within a few pixels of
//                             a face edge are read by a ring, and for the others the lane is a copy.  No atomics, no
//                             workspace, every element stored once by its own lane.
//   cube_points_records_kernel  one lane per point of a point set: the direction the host gives -> the record on the padded
//                             stack, so that the sphere-sampled metrics (sphere_points.hip) read a cube picture (§4k).
#include <algorithm>
#include <vector>

#include "sphere_sampler.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = kBlock / kTileW;
constexpr int kPad = PCONV_CUBE_PAD;

// forward, right, up of the six faces (the table of include/pconv_hip.h), as kernel arguments would cost 54 doubles:
// the entries are 0 and +-1, so they are spelt as a switch the compiler folds
struct Frame3 {
  double f[3], r[3], u[3];
};

__host__ __device__ inline Frame3 face_frame(int face) {
  switch (face) {
    case 0: return {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};     // F
    case 1: return {{0, 1, 0}, {-1, 0, 0}, {0, 0, 1}};    // R
    case 2: return {{-1, 0, 0}, {0, -1, 0}, {0, 0, 1}};   // B
    case 3: return {{0, -1, 0}, {1, 0, 0}, {0, 0, 1}};    // L
    case 4: return {{0, 0, 1}, {0, 1, 0}, {-1, 0, 0}};    // U
    default: return {{0, 0, -1}, {0, 1, 0}, {1, 0, 0}};   // D
  }
}

// the axis of largest magnitude, ties in the order x, y, z; the sign picks the face
__host__ __device__ inline int face_of(double x, double y, double z) {
  const double ax = fabs(x), ay = fabs(y), az = fabs(z);
  if (ax >= ay && ax >= az) return x >= 0.0 ? 0 : 2;
  if (ay >= az) return y >= 0.0 ? 1 : 3;
  return z >= 0.0 ? 4 : 5;
}

__device__ __forceinline__ double plane_of(int kind, double s) { return kind == PCONV_CUBE_EAC ? tan((kPi / 4.0) * s) : s; }
__device__ __forceinline__ double face_of_plane(int kind, double p) { return kind == PCONV_CUBE_EAC ? (4.0 / kPi) * atan(p) : p; }

__global__ __launch_bounds__(kBlock) void cube_from_erp_map_kernel(int2 *__restrict__ map, int kind, int gs, int h, int w,
                                                                   int tiles) {
  const int R = blockIdx.x / tiles;  // 0 .. 6 gs - 1
  const int q = (blockIdx.x - R * tiles) * kBlock + threadIdx.x;
  if (q >= gs) return;
  const int face = R / gs, r = R - face * gs;
  const double ps = plane_of(kind, 2.0 * (q + 0.5) / gs - 1.0);
  const double pt = plane_of(kind, 1.0 - 2.0 * (r + 0.5) / gs);
  const Frame3 B = face_frame(face);
  const double sx = B.f[0] + ps * B.r[0] + pt * B.u[0];
  const double sy = B.f[1] + ps * B.r[1] + pt * B.u[1];
  const double sz = B.f[2] + ps * B.r[2] + pt * B.u[2];
  map[(long long)R * gs + q] = record_of_direction(sx, sy, sz, h, w);
}

__global__ __launch_bounds__(kBlock) void cube_to_erp_map_kernel(int2 *__restrict__ map, int kind, int a, int gh, int gw,
                                                                 int tiles) {
  const int j = blockIdx.x / tiles;
  const int i = (blockIdx.x - j * tiles) * kBlock + threadIdx.x;
  if (i >= gw) return;
  const double theta = ((i + 0.5) / gw - 0.5) * (2.0 * kPi);
  const double phi = (0.5 - (j + 0.5) / gh) * kPi;
  const double cp = cos(phi), sp = sin(phi);
  const double dx = cp * cos(theta), dy = cp * sin(theta), dz = sp;
  const int g = face_of(dx, dy, dz);
  const Frame3 B = face_frame(g);
  const double along = dx * B.f[0] + dy * B.f[1] + dz * B.f[2];
  const double s = face_of_plane(kind, (dx * B.r[0] + dy * B.r[1] + dz * B.r[2]) / along);
  const double t = face_of_plane(kind, (dx * B.u[0] + dy * B.u[1] + dz * B.u[2]) / along);
  // inside the face: |s|, |t| <= 1 up to the rounding of atan, so the clamp moves nothing but keeps every footprint
  // inside its own padded face whatever the arithmetic did
  const double lo = -0.5, hi = a - 0.5;
  const double u = fmin(fmax((s + 1.0) * a / 2.0 - 0.5, lo), hi);
  const double v = fmin(fmax((1.0 - t) * a / 2.0 - 0.5, lo), hi);
  const int A = a + 2 * kPad;
  map[(long long)j * gw + i] = make_int2((int)rint((u + kPad) * kPhases), (int)rint((v + kPad + (double)g * A) * kPhases));
}

// one lane per point: the record of a direction on the padded stack.  The position is cube_to_erp_map_kernel's, word for
// word, from a direction the host computed (no sin / cos here, and for CMP no transcendental at all); the upper clamp is
// 1/256 pixel tighter, so that the nearest pixel of the record is always a pixel of the face itself.
__global__ __launch_bounds__(kBlock) void cube_points_records_kernel(const double *__restrict__ dirs, int2 *__restrict__ records,
                                                                     long long P, int kind, int a) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= P) return;
  const double dx = dirs[3 * k], dy = dirs[3 * k + 1], dz = dirs[3 * k + 2];
  const int g = face_of(dx, dy, dz);
  const Frame3 B = face_frame(g);
  const double along = dx * B.f[0] + dy * B.f[1] + dz * B.f[2];
  const double s = face_of_plane(kind, (dx * B.r[0] + dy * B.r[1] + dz * B.r[2]) / along);
  const double t = face_of_plane(kind, (dx * B.u[0] + dy * B.u[1] + dz * B.u[2]) / along);
  // fmax / fmin return the other operand for a NaN (a zero direction): every record stays inside its padded face
  const double lo = -0.5, hi = a - 0.5 - 1.0 / kPhases;
  const double u = fmin(fmax((s + 1.0) * a / 2.0 - 0.5, lo), hi);
  const double v = fmin(fmax((1.0 - t) * a / 2.0 - 0.5, lo), hi);
  const int A = a + 2 * kPad;
  records[k] = make_int2((int)rint((u + kPad) * kPhases), (int)rint((v + kPad + (double)g * A) * kPhases));
}

__device__ __forceinline__ float lerp_rn(float x0, float x1, float f) {
  return __fadd_rn(x0, __fmul_rn(f, __fsub_rn(x1, x0)));
}

__global__ __launch_bounds__(kBlock) void cube_pad_f32_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                              const int *__restrict__ table, int a, int pad, int tiles) {
  const int A = a + 2 * pad;
  const int ty = blockIdx.x / tiles;
  const int Q = (blockIdx.x - ty * tiles) * kTileW + (threadIdx.x % kTileW);
  const int row = ty * kTileH + threadIdx.x / kTileW;  // 0 .. 6 A - 1
  if (Q >= A || row >= 6 * A) return;
  const int face = row / A, R = row - face * A;
  const float *src = in + (long long)blockIdx.y * 6 * a * a;   // a plane is below 2^29 floats
  float *dst = out + (long long)blockIdx.y * 6 * A * A + (row * A + Q);
  const int r = R - pad, c = Q - pad;
  if (r >= 0 && r < a && c >= 0 && c < a) {
    *dst = src[(face * a + r) * a + c];
    return;
  }
  // ring order: the pixels of the padded face outside its interior, row after row, column after column
  int k;
  if (R < pad) k = R * A + Q;
  else if (R < pad + a) k = pad * A + (R - pad) * 2 * pad + (Q < pad ? Q : Q - a);
  else k = pad * A + 2 * pad * a + (R - pad - a) * A + Q;
  const int *rec = table + 3 * (face * (A * A - a * a) + k);
  // whatever the table holds is reduced to a position inside a face
  const int g = min(max(rec[0], 0), 5);
  const int x0 = min(max(rec[1] >> 8, 0), a - 1), y0 = min(max(rec[2] >> 8, 0), a - 1);
  const int x1 = min(x0 + 1, a - 1), y1 = min(y0 + 1, a - 1);
  const float fx = (float)record_phase(rec[1]) * (1.0f / kPhases), fy = (float)record_phase(rec[2]) * (1.0f / kPhases);
  const float *fsrc = src + g * a * a;
  const float top = lerp_rn(fsrc[y0 * a + x0], fsrc[y0 * a + x1], fx);
  const float bot = lerp_rn(fsrc[y1 * a + x0], fsrc[y1 * a + x1], fx);
  *dst = lerp_rn(top, bot, fy);
}

constexpr int kPlanes = 4;  // planes a lane carries through one walk of its list

// ring pixel k of a padded face (ring order: row after row, column after column, outside the interior) -> R * A + Q; the
// inverse of cube_pad_f32_kernel's count.  k in 0 .. A * A - a * a - 1
__host__ __device__ inline int ring_pixel(int k, int a, int pad) {
  const int A = a + 2 * pad, top = pad * A, sides = 2 * pad * a;
  if (k < top) return k;
  if (k < top + sides) {
    const int m = k - top, row = m / (2 * pad), j = m - row * 2 * pad;
    return (pad + row) * A + (j < pad ? j : j + a);
  }
  return (pad + a) * A + (k - top - sides);
}

__global__ __launch_bounds__(kBlock) void cube_pad_backward_f32_kernel(const float *__restrict__ gout, float *__restrict__ gin,
                                                                       const int *__restrict__ table,
                                                                       const int32_t *__restrict__ rev_start,
                                                                       const int32_t *__restrict__ rev_entry, int C, int a,
                                                                       int pad, int total) {
  const int A = a + 2 * pad, ring = A * A - a * a, pixels = 6 * a * a;
  const int d = blockIdx.x * kBlock + threadIdx.x;  // 6 a^2 < 2^29
  if (d >= pixels) return;
  const int groups = (C + kPlanes - 1) / kPlanes;
  const int frame = blockIdx.y / groups, c0 = (blockIdx.y - frame * groups) * kPlanes;
  const int planes = min(kPlanes, C - c0);
  const long long gplane = 6LL * A * A;
  const float *g = gout + ((long long)frame * C + c0) * gplane;
  float *dst = gin + ((long long)frame * C + c0) * pixels + d;
  const int lo = min(max(rev_start[d], 0), total), hi = min(max(rev_start[d + 1], 0), total);
  const int face = d / (a * a), r = (d - face * a * a) / a, c = d - (face * a + r) * a;
  const int own = (face * A + pad + r) * A + pad + c;
  float acc[kPlanes];
#pragma unroll
  for (int k = 0; k < kPlanes; k++) acc[k] = k < planes ? g[(long long)k * gplane + own] : 0.f;
  for (int at = lo; at < hi; at++) {
    const int e = rev_entry[at];
    if ((unsigned)e >= (unsigned)total) continue;  // whatever the list holds is reduced to an entry of the table
    const int i = e >> 2, corner = e & 3;
    const int *rec = table + 3 * i;
    const int px = record_phase(rec[1]), py = record_phase(rec[2]);
    const int cx = (corner & 1) ? px : kPhases - px, cy = (corner & 2) ? py : kPhases - py;
    const float coef = (float)(cx * cy) * (1.0f / (kPhases * kPhases));  // exact: cx * cy <= 2^16
    const int rf = i / ring;                                              // 0 .. 5, as i < 6 ring
    const int at_ring = rf * A * A + ring_pixel(i - rf * ring, a, pad);
#pragma unroll
    for (int k = 0; k < kPlanes; k++)
      if (k < planes) acc[k] = __fadd_rn(acc[k], __fmul_rn(g[(long long)k * gplane + at_ring], coef));
  }
#pragma unroll
  for (int k = 0; k < kPlanes; k++)
    if (k < planes) dst[(long long)k * pixels] = acc[k];
}

int kind_ok(const char *what, int kind) {
  PCONV_REQUIRE(kind == PCONV_CUBE_CMP || kind == PCONV_CUBE_EAC, "%s: kind %d is neither PCONV_CUBE_CMP (1) nor PCONV_CUBE_EAC (2)",
                what, kind);
  return PCONV_OK;
}

int face_ok(const char *what, int a) {
  PCONV_REQUIRE(a >= 2 && a <= PCONV_CUBE_MAX_FACE, "%s: a face size of %d is outside 2 .. %d (the padded stack stays below 2^31 "
                "bytes)", what, a, PCONV_CUBE_MAX_FACE);
  return PCONV_OK;
}

int ss_ok(const char *what, int ss) {
  PCONV_REQUIRE(ss >= 1 && ss <= PCONV_VIEWPORT_MAX_SS, "%s: ss = %d supersampling is outside 1 .. %d", what, ss,
                PCONV_VIEWPORT_MAX_SS);
  return PCONV_OK;
}

}  // namespace

extern "C" int pconv_host_cube_face_of(double x, double y, double z) { return face_of(x, y, z); }

extern "C" int pconv_cube_from_erp_map(int32_t *map, int kind, int a, int ss, int h, int w, void *stream) {
  const char *what = "cube_from_erp_map";
  PCONV_REQUIRE(map, "%s: null pointer", what);
  if (kind_ok(what, kind) != PCONV_OK || face_ok(what, a) != PCONV_OK || ss_ok(what, ss) != PCONV_OK ||
      frame_ok(what, "source ", h, w) != PCONV_OK || aligned8_ok(what, addr(map), "the map") != PCONV_OK)
    return PCONV_EINVAL;
  const long long gs = (long long)a * ss;
  PCONV_REQUIRE(8LL * 6 * gs * gs < (1LL << 31), "%s: a map of %lldx%lld records is 2^31 bytes or more", what, gs, 6 * gs);
  const int tiles = ((int)gs + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(cube_from_erp_map_kernel, dim3((unsigned)(6 * gs) * tiles), dim3(kBlock), 0, as_stream(stream),
                     reinterpret_cast<int2 *>(map), kind, (int)gs, h, w, tiles);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

extern "C" int pconv_cube_to_erp_map(int32_t *map, int kind, int a, int h, int w, int ss, void *stream) {
  const char *what = "cube_to_erp_map";
  PCONV_REQUIRE(map, "%s: null pointer", what);
  if (kind_ok(what, kind) != PCONV_OK || face_ok(what, a) != PCONV_OK || ss_ok(what, ss) != PCONV_OK ||
      frame_ok(what, "view ", h, w) != PCONV_OK || aligned8_ok(what, addr(map), "the map") != PCONV_OK)
    return PCONV_EINVAL;
  const long long gh = (long long)h * ss, gw = (long long)w * ss;
  PCONV_REQUIRE(8LL * gh * gw < (1LL << 31), "%s: a map of %lldx%lld records is 2^31 bytes or more", what, gw, gh);
  const int tiles = ((int)gw + kBlock - 1) / kBlock;  // gh * tiles < 2^28 / 256 + 2^22
  hipLaunchKernelGGL(cube_to_erp_map_kernel, dim3((unsigned)gh * tiles), dim3(kBlock), 0, as_stream(stream),
                     reinterpret_cast<int2 *>(map), kind, a, (int)gh, (int)gw, tiles);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

extern "C" int pconv_cube_points_records(const double *dirs, int32_t *records, long long P, int kind, int a, void *stream) {
  const char *what = "cube_points_records";
  PCONV_REQUIRE(dirs && records, "%s: null pointer", what);
  if (kind_ok(what, kind) != PCONV_OK || face_ok(what, a) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(P >= 1 && P <= (1LL << 28) - 1, "%s: %lld points, 1 .. 2^28 - 1 expected", what, P);
  if (aligned8_ok(what, addr(dirs) | addr(records), "the directions and the records") != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(addr(dirs) >= addr(records) + (uintptr_t)(8 * P) || addr(records) >= addr(dirs) + (uintptr_t)(24 * P),
                "%s: the records overlap the directions", what);
  const long long blocks = (P + kBlock - 1) / kBlock;  // below 2^20
  hipLaunchKernelGGL(cube_points_records_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), dirs,
                     reinterpret_cast<int2 *>(records), P, kind, a);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

namespace {

// a face size and a depth whose padded stack stays below 2^31 bytes
int depth_ok(const char *what, int a, int depth) {
  if (face_ok(what, a) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(depth >= 1 && depth <= PCONV_CUBE_MAX_DEPTH, "%s: a depth of %d is outside 1 .. %d", what, depth, PCONV_CUBE_MAX_DEPTH);
  const int A = a + 2 * depth;
  PCONV_REQUIRE(24LL * A * A < (1LL << 31), "%s: a face size of %d continued by %d: the padded stack is 2^31 bytes or more", what, a,
                depth);
  return PCONV_OK;
}

// the face continuation of any depth: pconv_cube_pad_f32 is depth PCONV_CUBE_PAD, where face_ok has bounded the stack
int cube_pad(const char *what, const float *in, float *out, const int32_t *table, int n, int c, int a, int depth, void *stream) {
  PCONV_REQUIRE(in && out && table, "%s: null pointer", what);
  if (planes_ok(what, n, c) != PCONV_OK || depth_ok(what, a, depth) != PCONV_OK) return PCONV_EINVAL;
  const int A = a + 2 * depth;
  PCONV_REQUIRE(((addr(in) | addr(out) | addr(table)) & 3) == 0, "%s: the tensors and the table must be 4-byte aligned", what);
  PCONV_REQUIRE(in != out, "%s: in and out must be distinct (the ring reads the faces)", what);
  const int tiles = (A + kTileW - 1) / kTileW;
  const long long groups = (long long)tiles * ((6 * A + kTileH - 1) / kTileH);  // below 2^29 / 256 + 6 A
  hipLaunchKernelGGL(cube_pad_f32_kernel, dim3((unsigned)groups, (unsigned)(n * c)), dim3(kBlock), 0, as_stream(stream), in, out,
                     table, a, depth, tiles);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

}  // namespace

extern "C" int pconv_cube_pad_f32(const float *in, float *out, const int32_t *table, int n, int c, int a, void *stream) {
  return cube_pad("cube_pad_f32", in, out, table, n, c, a, kPad, stream);
}

extern "C" int pconv_cube_pad_depth_f32(const float *in, float *out, const int32_t *table, int n, int c, int a, int depth,
                                        void *stream) {
  return cube_pad("cube_pad_depth_f32", in, out, table, n, c, a, depth, stream);
}

extern "C" long long pconv_host_cube_pad_reverse_size(int a, int depth) {
  if (depth_ok("cube_pad_reverse_size", a, depth) != PCONV_OK) return PCONV_EINVAL;
  const long long A = a + 2 * depth;
  return 24LL * (A * A - (long long)a * a);  // below 24 A^2 < 2^31
}

// Transpose of the face continuation as a CSR list per pixel of the face stack (pconv_cube_pad_backward_f32): the walk --
// ring pixel i ascending, corner 0 .. 3 = (y0, x0), (y0, x1), (y1, x0), (y1, x1) -- sorted by the pixel the corner reads
// with a stable counting sort, so every list ascends.  The face and the four positions are reduced exactly as
// cube_pad_f32_kernel reduces them.  Corners that coincide, and corners that weigh 0, are entries of their own.
extern "C" int pconv_host_cube_pad_reverse(const int32_t *table, int a, int depth, int32_t *rev_start, int32_t *rev_entry) {
  const char *what = "cube_pad_reverse";
  PCONV_REQUIRE(table && rev_start && rev_entry, "%s: null pointer", what);
  const long long total = pconv_host_cube_pad_reverse_size(a, depth);
  if (total < 0) return PCONV_EINVAL;
  const size_t keys = 6 * (size_t)a * a, rings = (size_t)(total / 4);
  std::vector<int32_t> fill(keys + 1, 0);
  for (int pass = 0; pass < 2; pass++) {
    for (size_t i = 0; i < rings; i++) {
      const int32_t *rec = table + 3 * i;
      const int g = std::min(std::max(rec[0], 0), 5);
      const int x0 = std::min(std::max(rec[1] >> 8, 0), a - 1), y0 = std::min(std::max(rec[2] >> 8, 0), a - 1);
      const int xs[2] = {x0, std::min(x0 + 1, a - 1)}, ys[2] = {y0, std::min(y0 + 1, a - 1)};
      for (int corner = 0; corner < 4; corner++) {
        const size_t d = ((size_t)g * a + ys[corner >> 1]) * a + xs[corner & 1];
        if (pass == 0) fill[d + 1]++;
        else rev_entry[fill[d]++] = (int32_t)(4 * i + corner);
      }
    }
    if (pass == 0) {
      for (size_t k = 0; k < keys; k++) fill[k + 1] += fill[k];
      for (size_t k = 0; k <= keys; k++) rev_start[k] = fill[k];
    }
  }
  return (int)total;
}

extern "C" int pconv_cube_pad_backward_f32(const float *gout, float *gin, const int32_t *table, const int32_t *rev_start,
                                           const int32_t *rev_entry, int n, int c, int a, int depth, void *stream) {
  const char *what = "cube_pad_backward_f32";
  PCONV_REQUIRE(gout && gin && table, "%s: null pointer", what);
  PCONV_REQUIRE(rev_start && rev_entry, "%s: null list pointer", what);
  if (planes_ok(what, n, c) != PCONV_OK || depth_ok(what, a, depth) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(((addr(gout) | addr(gin) | addr(table) | addr(rev_start) | addr(rev_entry)) & 3) == 0,
                "%s: the tensors, the table and the lists must be 4-byte aligned", what);
  PCONV_REQUIRE(gin != gout, "%s: gin and gout must be distinct (a pixel reads its neighbours' rings)", what);
  const long long total = pconv_host_cube_pad_reverse_size(a, depth);
  const int groups = (c + kPlanes - 1) / kPlanes;  // n * groups <= n * C <= 65535
  hipLaunchKernelGGL(cube_pad_backward_f32_kernel, dim3((unsigned)((6 * a * a + kBlock - 1) / kBlock), (unsigned)(n * groups)),
                     dim3(kBlock), 0, as_stream(stream), gout, gin, table, rev_start, rev_entry, c, a, depth, (int)total);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}
