// Predicted meshes to pixels: a batched, deterministic triangle rasteriser with an exact coverage rule and the shading / compositing
// kernel of the overlays.  Stands in for the reference's pytorch3d renderer (lib/utils/render_fn.py, lib/dataset/base.py:472-500,632-688);
// the rules are this project's own and are stated in include/vpho_hip.h.
//   raster_setup_kernel   one thread per (image, face): project in fp64, snap to the 1/256-pixel lattice, orient, box -> one 48-byte record and its 8-byte box
//   raster_tile_kernel    one 256-thread workgroup per (image, 16 x 16 tile): walks the image's boxes 256 at a time, keeps the faces whose
//                         box touches the tile (ballot compaction into LDS, face order kept); each wave owns an 8 x 8 quadrant, each lane
//                         ONE pixel and its running (front, back) pair in registers -- a tile's faces are a serial chain, so the chain is
//                         kept short per wave; 64-bit integer edge functions, fp64 depth, no atomics
//   render_overlay_kernel one thread per pixel: nearer layer, face normal against the viewing ray, blend over the de-normalised image
// Every index into the maps is checked against H and W; the face and vertex indices come from a table the caller validated.
#include "common.h"
#include "../../include/vpho_hip.h"
#include <cstdint>

namespace {

constexpr int TILE = 16;                    // pixels per tile side: four waves, each an 8 x 8 quadrant, one pixel per lane
constexpr int CHUNK = 256;                  // threads of a tile's workgroup = boxes tested per round, one per thread
constexpr int MAX_SIDE = 2048;
constexpr double SNAP = 256.0, SNAP_MAX = 1073741824.0;                     // 2^30
constexpr unsigned BOX_NONE = 0xFFFFu;                                       // low column of a dropped face: beyond every tile

struct FaceRec {                            // 48 bytes
    int x0, y0, x1, y1, x2, y2;             // snapped corners, oriented: (x1 - x0) (y2 - y0) - (y1 - y0) (x2 - x0) > 0
    float z0, z1, z2;
    unsigned bx, by;                        // pixel columns / rows whose centres the box holds, clipped to the image: lo | hi << 16
    int pad;
};
static_assert(sizeof(FaceRec) == 48, "record size is part of vpho_mesh_raster_bytes");

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for NaN and infinities

__global__ __launch_bounds__(256) void raster_setup_kernel(const vpho_mesh_table t, const float* __restrict__ verts, int Vmax, const int* __restrict__ mesh_id,
                                                           const double* __restrict__ K, int n, int H, int W, int stride, double z_near,
                                                           FaceRec* __restrict__ rec, uint2* __restrict__ box) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)n * stride) return;
    const int img = (int)(id / stride), f = (int)(id % stride);
    const int m = mesh_id[img];
    if (m < 0 || m >= t.M) return;                                            // the tile kernel reads no record of such an image
    const int f0 = t.face_offset[m], nf = t.face_offset[m + 1] - f0;
    if (f >= nf) return;
    const int* fi = t.faces + 3ll * (f0 + f);
    const float* vb = verts + (long long)img * Vmax * 3;
    const double* k = K + 9ll * img;
    long long sx[3], sy[3];
    float z[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = vb + 3ll * fi[c];
        const double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
        z[c] = p[2];
        ok = ok && finite_d(X) && finite_d(Y) && finite_d(Z) && Z > z_near;
        const double u = (k[0] * X + k[1] * Y) / Z + k[2];
        const double v = (k[4] * Y) / Z + k[5];
        const double su = rint(u * SNAP), sv = rint(v * SNAP);                // ties to even
        ok = ok && fabs(su) <= SNAP_MAX && fabs(sv) <= SNAP_MAX;              // a NaN fails both
        sx[c] = ok ? (long long)su : 0;
        sy[c] = ok ? (long long)sv : 0;
    }
    FaceRec r;
    r.bx = BOX_NONE; r.by = BOX_NONE; r.pad = 0;
    r.x0 = r.y0 = r.x1 = r.y1 = r.x2 = r.y2 = 0;
    r.z0 = r.z1 = r.z2 = 1.f;
    const long long area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);      // |.| <= 2^62
    if (ok && area != 0) {
        const bool swap = area < 0;                                           // both windings count: corners 1 and 2 change places
        const long long minx = min(sx[0], min(sx[1], sx[2])), maxx = max(sx[0], max(sx[1], sx[2]));
        const long long miny = min(sy[0], min(sy[1], sy[2])), maxy = max(sy[0], max(sy[1], sy[2]));
        // pixel p has its centre at lattice 256 p + 128: p >= (min - 128) / 256 rounded up, p <= (max - 128) / 256 rounded down
        const long long xlo = max((minx + 127) >> 8, 0ll), xhi = min((maxx - 128) >> 8, (long long)W - 1);
        const long long ylo = max((miny + 127) >> 8, 0ll), yhi = min((maxy - 128) >> 8, (long long)H - 1);
        if (xlo <= xhi && ylo <= yhi) {
            r.x0 = (int)sx[0]; r.y0 = (int)sy[0];
            r.x1 = (int)(swap ? sx[2] : sx[1]); r.y1 = (int)(swap ? sy[2] : sy[1]);
            r.x2 = (int)(swap ? sx[1] : sx[2]); r.y2 = (int)(swap ? sy[1] : sy[2]);
            r.z0 = z[0]; r.z1 = swap ? z[2] : z[1]; r.z2 = swap ? z[1] : z[2];
            r.bx = (unsigned)xlo | ((unsigned)xhi << 16);
            r.by = (unsigned)ylo | ((unsigned)yhi << 16);
        }
    }
    rec[(long long)img * stride + f] = r;
    box[(long long)img * stride + f] = make_uint2(r.bx, r.by);
}

// top-left rule on an oriented face (y grows downwards): an edge (dx, dy) owns the centres that lie on it when it is a left edge (dy < 0)
// or a top edge (dy == 0, dx > 0); E >= 0 on such an edge, E > 0 on the others, as (E + bias) >= 0 with bias 0 / -1
__device__ __forceinline__ long long edge_bias(long long dx, long long dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0ll : -1ll; }

struct PixelState { double zf, zb; int ff, fb; };

// perspective-correct depth at a covered centre from its three edge values (include/vpho_hip.h has the operation order)
__device__ __forceinline__ double face_depth(long long e0, long long e1, long long e2, double area, double z0, double z1, double z2) {
    const double w0 = (double)e0 / area, w1 = (double)e1 / area, w2 = (double)e2 / area;
    const double inv = (w0 / z0 + w1 / z1) + w2 / z2;
    return 1.0 / inv;
}
__device__ __forceinline__ void keep_depth(PixelState& s, double z, int face) {
    if (z < s.zf) { s.zf = z; s.ff = face; }                                  // faces arrive in ascending index: the first of equals stays
    if (z > s.zb) { s.zb = z; s.fb = face; }
}

__global__ __launch_bounds__(CHUNK) void raster_tile_kernel(const vpho_mesh_table t, const int* __restrict__ mesh_id, const FaceRec* __restrict__ rec, const uint2* __restrict__ box, int stride,
                                                         int H, int W, int tiles_x, int tiles, float* __restrict__ depth_front,
                                                         float* __restrict__ depth_back, int* __restrict__ face_front, int* __restrict__ face_back) {
    __shared__ int4 sh[3 * CHUNK];                                            // a record as three 16-byte words
    __shared__ int shf[CHUNK];
    __shared__ int wave_hits[CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int tx0 = (tile % tiles_x) * TILE, ty0 = (tile / tiles_x) * TILE;
    const int qx0 = tx0 + 8 * (wave & 1), qy0 = ty0 + 8 * (wave >> 1);       // the wave's 8 x 8 quadrant
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);                 // the lane's pixel
    const int m = mesh_id[img];
    int nf = 0;
    if (m >= 0 && m < t.M) nf = min(t.face_offset[m + 1] - t.face_offset[m], stride);
    const int4* rp = reinterpret_cast<const int4*>(rec + (long long)img * stride);
    const uint2* bp = box + (long long)img * stride;
    PixelState s{INFINITY, -INFINITY, -1, -1};
    const long long cx = 256ll * px + 128, cy = 256ll * py + 128;
    // every tile of an image walks all its faces: the walk reads the 8-byte boxes only (one chunk ahead), the 48-byte record of a survivor
    uint2 next = tid < nf ? bp[tid] : make_uint2(BOX_NONE, BOX_NONE);
    for (int base = 0; base < nf; base += CHUNK) {                            // workgroup-uniform
        const int f = base + tid;
        const uint2 b = next;
        next = f + CHUNK < nf ? bp[f + CHUNK] : make_uint2(BOX_NONE, BOX_NONE);
        const int bxlo = (int)(b.x & 0xFFFFu), bxhi = (int)(b.x >> 16), bylo = (int)(b.y & 0xFFFFu), byhi = (int)(b.y >> 16);
        const bool hit = bxlo <= tx0 + TILE - 1 && bxhi >= tx0 && bylo <= ty0 + TILE - 1 && byhi >= ty0;       // a dropped face has lo = 0xFFFF
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, cnt = 0;                                              // survivors keep their order: waves in turn, lanes in turn
#pragma unroll
        for (int w = 0; w < CHUNK / 64; ++w) {
            const int h = wave_hits[w];
            before += w < wave ? h : 0;
            cnt += h;
        }
        if (hit) {                                                            // hit implies f < nf
            const int slot = before + __popcll(mask & ((1ull << lane) - 1ull));
            sh[3 * slot] = rp[3ll * f]; sh[3 * slot + 1] = rp[3ll * f + 1]; sh[3 * slot + 2] = rp[3ll * f + 2];      // x0 y0 x1 y1 | x2 y2 z0 z1 | z2 bx by pad
            shf[slot] = f;
        }
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const int4 q2 = sh[3 * i + 2];                                    // every lane reads the same record
            const int xlo = q2.y & 0xFFFF, xhi = (int)((unsigned)q2.y >> 16), ylo = q2.z & 0xFFFF, yhi = (int)((unsigned)q2.z >> 16);
            if (px < xlo || px > xhi || py < ylo || py > yhi) continue;       // a face that misses the whole quadrant costs its wave nothing more
            const int face = shf[i];
            const int4 q0 = sh[3 * i], q1 = sh[3 * i + 1];
            struct { long long x0, y0, x1, y1, x2, y2; float z0, z1, z2; } q{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, __int_as_float(q1.z), __int_as_float(q1.w), __int_as_float(q2.x)};
            const long long dx0 = q.x2 - q.x1, dy0 = q.y2 - q.y1;       // edge 0: corner 1 -> 2, opposite corner 0
            const long long dx1 = q.x0 - q.x2, dy1 = q.y0 - q.y2;       // edge 1: corner 2 -> 0
            const long long dx2 = q.x1 - q.x0, dy2 = q.y1 - q.y0;       // edge 2: corner 0 -> 1
            const long long e0 = dx0 * (cy - q.y1) - dy0 * (cx - q.x1);
            const long long e1 = dx1 * (cy - q.y2) - dy1 * (cx - q.x2);
            const long long e2 = dx2 * (cy - q.y0) - dy2 * (cx - q.x0);
            const long long b0 = edge_bias(dx0, dy0), b1 = edge_bias(dx1, dy1), b2 = edge_bias(dx2, dy2);
            const double area = (double)((e0 + e1) + e2);                     // the doubled area, the same at every centre
            const double z0 = (double)q.z0, z1 = (double)q.z1, z2 = (double)q.z2;
            if (((e0 + b0) | (e1 + b1) | (e2 + b2)) >= 0) keep_depth(s, face_depth(e0, e1, e2, area, z0, z1, z2), face);
        }
        __syncthreads();
    }
    if (px < W && py < H) {
        const long long o = ((long long)img * H + py) * W + px;
        if (depth_front) depth_front[o] = s.ff >= 0 ? (float)s.zf : 0.f;
        if (depth_back) depth_back[o] = s.fb >= 0 ? (float)s.zb : 0.f;
        if (face_front) face_front[o] = s.ff;
        if (face_back) face_back[o] = s.fb;
    }
}

// ---------------------------------------------------------------------------------------------------------------- overlay
struct OverlayArgs {
    const float* image; const double* K; vpho_render_layer hand, obj; int has_hand, has_obj;
    double mean[3], sd[3], ambient; int n, H, W; unsigned char* out;
};

// shade of the layer's face under pixel (x, y) of image `img`; false when the layer has no usable face there
__device__ __forceinline__ double face_shade(const vpho_render_layer& L, int img, int face, double rx, double ry, double ambient) {
    const int m = L.mesh_id[img];
    if (m < 0 || m >= L.M) return ambient;
    const int f0 = L.face_offset[m];
    if (face >= L.face_offset[m + 1] - f0) return ambient;
    const int* fi = L.faces + 3ll * (f0 + face);
    const float* vb = L.verts + (long long)img * L.Vmax * 3;
    const float *p0 = vb + 3ll * fi[0], *p1 = vb + 3ll * fi[1], *p2 = vb + 3ll * fi[2];
    const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
    const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
    const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double n2 = (nx * nx + ny * ny) + nz * nz;
    if (!(n2 > 0.0)) return ambient;                                         // a zero (or NaN) normal: the ambient term only
    const double dot = (nx * rx + ny * ry) + nz;
    const double d2 = (rx * rx + ry * ry) + 1.0;
    return ambient + (1.0 - ambient) * (fabs(dot) / (sqrt(n2) * sqrt(d2)));
}

__device__ __forceinline__ unsigned char to_byte(double v) {
    if (!(v > 0.0)) return 0;                                                 // a NaN becomes 0
    return (unsigned char)rint(fmin(v, 255.0));                               // half to even
}

__global__ __launch_bounds__(256) void render_overlay_kernel(const OverlayArgs a) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long hw = (long long)a.H * a.W;
    if (id >= (long long)a.n * hw) return;
    const int img = (int)(id / hw);
    const long long pix = id % hw;
    const int y = (int)(pix / a.W), x = (int)(pix % a.W);
    int hf = -1, of = -1;
    float hd = 0.f, od = 0.f;
    if (a.has_hand) { hf = a.hand.face_front[id]; hd = a.hand.depth_front[id]; }
    if (a.has_obj) { of = a.obj.face_front[id]; od = a.obj.depth_front[id]; }
    const bool hand = hf >= 0 && (of < 0 || hd <= od);                        // the hand wins an exact tie
    const bool obj = !hand && of >= 0;
    double bg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) bg[c] = ((double)a.image[((long long)img * 3 + c) * hw + pix] * a.sd[c] + a.mean[c]) * 255.0;
    double o[3] = {bg[0], bg[1], bg[2]};
    if (hand || obj) {
        const vpho_render_layer& L = hand ? a.hand : a.obj;
        const double* k = a.K + 9ll * img;
        const double ry = (((double)y + 0.5) - k[5]) / k[4];                  // d = K^-1 (x + 0.5, y + 0.5, 1) of the upper-triangular K
        const double rx = ((((double)x + 0.5) - k[2]) - k[1] * ry) / k[0];
        const double shade = face_shade(L, img, hand ? hf : of, rx, ry, a.ambient);
        const double op = (double)L.opacity;
        const double col[3] = {(double)L.red, (double)L.green, (double)L.blue};
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (op * shade) * col[c] + (1.0 - op) * bg[c];
    }
    unsigned char* q = a.out + id * 3;
    q[0] = to_byte(o[0]); q[1] = to_byte(o[1]); q[2] = to_byte(o[2]);
}

int check_table(const vpho_mesh_table* t, const char* who) {
    VPHO_REQUIRE(t && t->faces && t->face_offset && t->vert_count && t->M > 0, "%s: NULL table or a table without meshes", who);
    return 0;
}

}  // namespace

extern "C" long long vpho_mesh_raster_bytes(int n, int face_stride) {
    if (n < 0 || face_stride < 0) return -1;
    return (long long)n * face_stride * (long long)(sizeof(FaceRec) + sizeof(uint2));     // the records, then the boxes once more on their own
}

extern "C" int vpho_mesh_raster_f32(const vpho_mesh_table* t, const float* verts, int Vmax, const int* mesh_id, const double* K, int n, int H, int W,
                                    int face_stride, double z_near, float* depth_front, float* depth_back, int* face_front, int* face_back,
                                    void* workspace, void* stream) {
    VPHO_REQUIRE(n >= 0 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "vpho_mesh_raster_f32: bad size (n %d, H %d, W %d; sides 1 .. %d)", n, H, W, MAX_SIDE);
    VPHO_REQUIRE(z_near > 0.0 && z_near < 1e30, "vpho_mesh_raster_f32: z_near must be positive and finite");
    if (n == 0) return 0;
    if (check_table(t, "vpho_mesh_raster_f32")) return 1;
    VPHO_REQUIRE(verts && mesh_id && K && Vmax > 0 && face_stride >= 0, "vpho_mesh_raster_f32: NULL verts / mesh_id / K, or a bad Vmax / face_stride");
    VPHO_REQUIRE(face_stride == 0 || (workspace && (uintptr_t)workspace % 16 == 0), "vpho_mesh_raster_f32: NULL or not 16-byte aligned workspace (vpho_mesh_raster_bytes)");
    const int tiles_x = (W + TILE - 1) / TILE, tiles = tiles_x * ((H + TILE - 1) / TILE);
    VPHO_REQUIRE((long long)n * tiles < (1ll << 31) && ((long long)n * face_stride + 255) / 256 < (1ll << 31), "vpho_mesh_raster_f32: too many tiles or faces for one launch");
    FaceRec* rec = (FaceRec*)workspace;
    uint2* box = (uint2*)(rec + (long long)n * face_stride);                  // 48 n face_stride is a multiple of 16
    const long long items = (long long)n * face_stride;
    if (items > 0) {
        hipLaunchKernelGGL(raster_setup_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *t, verts, Vmax, mesh_id, K, n, H, W,
                           face_stride, z_near, rec, box);
        if (int rc = vpho::check_launch("raster_setup_kernel")) return rc;
    }
    if (!depth_front && !depth_back && !face_front && !face_back) return 0;
    hipLaunchKernelGGL(raster_tile_kernel, dim3((unsigned)((long long)n * tiles)), dim3(CHUNK), 0, (hipStream_t)stream, *t, mesh_id, rec, box, face_stride, H, W, tiles_x,
                       tiles, depth_front, depth_back, face_front, face_back);
    return vpho::check_launch("raster_tile_kernel");
}

extern "C" int vpho_render_overlay_u8(const float* image, const float* mean_host, const float* std_host, const double* K, const vpho_render_layer* hand,
                                      const vpho_render_layer* obj, float ambient, int n, int H, int W, unsigned char* out, void* stream) {
    VPHO_REQUIRE(n >= 0 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "vpho_render_overlay_u8: bad size (n %d, H %d, W %d; sides 1 .. %d)", n, H, W, MAX_SIDE);
    VPHO_REQUIRE(ambient >= 0.f && ambient <= 1.f, "vpho_render_overlay_u8: ambient outside [0, 1]");
    if (n == 0) return 0;
    VPHO_REQUIRE(image && mean_host && std_host && out, "vpho_render_overlay_u8: NULL image / mean / std / out");
    VPHO_REQUIRE(K || (!hand && !obj), "vpho_render_overlay_u8: a layer without K");
    OverlayArgs a{};
    a.image = image; a.K = K; a.n = n; a.H = H; a.W = W; a.out = out; a.ambient = (double)ambient;
    for (int c = 0; c < 3; ++c) { a.mean[c] = (double)mean_host[c]; a.sd[c] = (double)std_host[c]; }
    const vpho_render_layer* in[2] = {hand, obj};
    for (int l = 0; l < 2; ++l) {
        const vpho_render_layer* L = in[l];
        if (!L) continue;
        VPHO_REQUIRE(L->depth_front && L->face_front && L->verts && L->mesh_id && L->faces && L->face_offset && L->Vmax > 0 && L->M > 0,
                     "vpho_render_overlay_u8: the %s layer has a NULL field or a bad size", l ? "object" : "hand");
        VPHO_REQUIRE(L->opacity >= 0.f && L->opacity <= 1.f, "vpho_render_overlay_u8: the %s layer's opacity is outside [0, 1]", l ? "object" : "hand");
        if (l) { a.obj = *L; a.has_obj = 1; } else { a.hand = *L; a.has_hand = 1; }
    }
    const long long total = (long long)n * H * W;
    VPHO_REQUIRE((total + 255) / 256 < (1ll << 31), "vpho_render_overlay_u8: too many pixels for one launch");
    hipLaunchKernelGGL(render_overlay_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return vpho::check_launch("render_overlay_kernel");
}
