// Scored scans as coloured triangle meshes, assembled on the device (docs/mesh.md): the organised cloud [n, H x W] float32, the
// score maps [n,H,W] f64 and (optionally) the region labels -> per image a dense run of 35-byte PLY vertex records (x y z, nx ny nz,
// red green blue, score, region) and of 13-byte face records (3, a, b, c), each in the image's fixed slot of a byte buffer.
// Vertices are the valid points in raster order; cell (y, x) gives T0 = (y,x),(y,x+1),(y+1,x+1) and T1 = (y,x),(y+1,x+1),(y+1,x),
// a triangle is emitted iff its vertices are valid and its edges have d2 = (dx dx + dy dy) + dz dz <= max_edge2; a vertex normal is
// the sum of (b - a) x (c - a) over its emitted incident triangles in a fixed order, normalised.  Every floating-point step is one
// float64 operation in the written order (the file is compiled with -ffp-contract=off); no float goes through an atomic.
//
// grid (ceil(H W / 1024), n), 256 lanes, a lane takes pixels 4t .. 4t + 3 of its chunk, so thread order is raster order.
//   mesh_count_kernel   per chunk the number of vertices and faces -> chunks [n,C,2]; per image n_vert, n_face, bad, nan (integer
//                       atomics on counts, zeroed by a memset in front)
//   mesh_vertex_kernel  rank = the chunks in front + an exclusive scan over the workgroup; writes vidx and the vertex records
//   mesh_face_kernel    the same ranking over the emitted triangles; reads vidx, writes the face records
// A workgroup's records are contiguous in the output.  kStage: they are put together in LDS at the byte phase of their global
// address and written as whole dwords, head and tail bytes guarded; otherwise every byte is a store of its own to global memory.
// Reads: cloud, maps, labels and backgrounds below H W of the image (a neighbour outside the frame is an invalid point and is
// not read).  Writes: vidx below H W; records below the image's counted vertices / faces, which never exceed its slot.
#include "block_scan.h"
#include "cloud.h"
#include "frames.h"
#include "launch.h"
#include "overlay_color.h"

namespace {

constexpr int kMeshMaxTotal = 1 << 24;   // n * H * W of one call: below the frames.h total, the record buffers are bytes
constexpr int kChunk = 1024;          // pixels of a workgroup: 256 lanes x 4
constexpr int kVertexBytes = 35;      // 6 floats, 3 bytes, 1 float, 1 int
constexpr int kFaceBytes = 13;        // the list length (3) and three int32
// true: records staged in LDS and stored as dwords; false: byte stores.  Staged is 1.1 to 1.5 times faster (docs/mesh.md has the A/B)
constexpr bool kStageDefault = true;

struct MeshArgs {
    Cloud c;
    const double* maps;
    const double* lohi;
    const void* bg;
    const uint8_t* lut;
    const uint8_t* alpha;
    const int32_t* labels;      // null: region 0
    const int32_t* chunks;
    int32_t* vidx;
    uint8_t* vbuf;
    uint8_t* fbuf;
    double max2;
    double mean[3], stdv[3];
    int H, W, C;
    int lohi_per_image, bg_kind, flip;
};

__device__ __forceinline__ bool edge_ok(const Pt& p, const Pt& q, double max2)
{
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= max2;
}

// the point of pixel (y, x), or an invalid one outside the frame
__device__ __forceinline__ Pt pt_at(const Cloud& c, size_t cbase, int y, int x, int H, int W)
{
    if (y < 0 || y >= H || x < 0 || x >= W) return {0.f, 0.f, 0.f};
    return cloud_at(c, cbase, y * W + x);
}

// the emitted triangles of cell (y, x): bit 0 = T0, bit 1 = T1 (both hold the diagonal a - c)
__device__ __forceinline__ int cell_faces(const Cloud& cl, size_t cbase, int y, int x, int H, int W, double max2)
{
    if (y + 1 >= H || x + 1 >= W) return 0;
    const int q = y * W + x;
    const Pt a = cloud_at(cl, cbase, q), c = cloud_at(cl, cbase, q + W + 1);
    if (!valid_pt(a) || !valid_pt(c) || !edge_ok(a, c, max2)) return 0;
    const Pt b = cloud_at(cl, cbase, q + 1), d = cloud_at(cl, cbase, q + W);
    int m = 0;
    if (valid_pt(b) && edge_ok(a, b, max2) && edge_ok(b, c, max2)) m |= 1;
    if (valid_pt(d) && edge_ok(c, d, max2) && edge_ok(d, a, max2)) m |= 2;
    return m;
}

// n += (b - a) x (c - a) when the triangle a, b, c is emitted
__device__ __forceinline__ void tri_add(const Pt& a, const Pt& b, const Pt& c, double max2, double& nx, double& ny, double& nz)
{
    if (!(valid_pt(a) && valid_pt(b) && valid_pt(c) && edge_ok(a, b, max2) && edge_ok(b, c, max2) && edge_ok(c, a, max2))) return;
    const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
    const double vx = (double)c.x - (double)a.x, vy = (double)c.y - (double)a.y, vz = (double)c.z - (double)a.z;
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    nx = nx + cx, ny = ny + cy, nz = nz + cz;
}

__device__ __forceinline__ void put32(uint8_t* d, uint32_t v)
{
    d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8), d[2] = (uint8_t)(v >> 16), d[3] = (uint8_t)(v >> 24);
}

// column `which` of chunks [n,C,2] summed over the chunks in front of this workgroup's
__device__ __forceinline__ int chunks_in_front(const int32_t* __restrict__ chunks, int C, int which, int* sh)
{
    const int32_t* row = chunks + (size_t)blockIdx.y * C * 2 + which;
    int v = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) v += row[j * 2];
    return block_sum(v, sh);
}

// The staged records of a workgroup, `bytes` of them from byte `start` (0..3) of sh, go to g0 (g0 & 3 == start): whole dwords
// where all four bytes are the workgroup's, single bytes at the head and the tail.  The caller has a barrier in front.
__device__ __forceinline__ void flush_staged(const uint32_t* sh, uint8_t* g0, int start, int bytes)
{
    uint8_t* ga = g0 - start;      // dword aligned
    const int end = start + bytes, nd = (end + 3) >> 2;
    for (int j = threadIdx.x; j < nd; j += 256) {
        const int lo = j * 4;
        if (lo >= start && lo + 4 <= end) {
            reinterpret_cast<uint32_t*>(ga)[j] = sh[j];
        } else {
            const uint8_t* sb = reinterpret_cast<const uint8_t*>(sh);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (lo + b >= start && lo + b < end) ga[lo + b] = sb[lo + b];
        }
    }
}

// grid (C, n): chunks [n,C,2] = vertices, faces of the chunk; counts [n,4] += n_vert, n_face, bad, nan
__global__ __launch_bounds__(256) void mesh_count_kernel(Cloud cl, const double* __restrict__ maps, int H, int W, int C, double max2,
                                                         int32_t* __restrict__ chunks, int32_t* __restrict__ counts)
{
    __shared__ int sh[4][4];
    const int tid = threadIdx.x, img = blockIdx.y, HW = H * W;
    const int p0 = ((int)blockIdx.x * 256 + tid) * 4;
    const size_t cbase = (size_t)img * 3 * HW;
    const double* __restrict__ m = maps + (size_t)img * HW;
    int nv = 0, nf = 0, bad = 0, nan = 0;
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p0 + k < HW) {
            const Pt p = cloud_at(cl, cbase, p0 + k);
            if (!finite3(p)) {
                ++bad;
            } else if (valid_pt(p)) {
                ++nv;
                const double s = m[p0 + k];
                nan += s != s;
            }
            nf += __popc(cell_faces(cl, cbase, y, x, H, W, max2));
        }
        if (++x == W) x = 0, ++y;
    }
    const int t0 = block_sum(nv, sh[0]), t1 = block_sum(nf, sh[1]), t2 = block_sum(bad, sh[2]), t3 = block_sum(nan, sh[3]);
    if (tid == 0) {
        int32_t* o = chunks + ((size_t)img * C + blockIdx.x) * 2;
        o[0] = t0, o[1] = t1;
        int32_t* cn = counts + (size_t)img * 4;
        if (t0) atomicAdd(cn + 0, t0);
        if (t1) atomicAdd(cn + 1, t1);
        if (t2) atomicAdd(cn + 2, t2);
        if (t3) atomicAdd(cn + 3, t3);
    }
}

template <bool kStage>
__global__ __launch_bounds__(256) void mesh_vertex_kernel(MeshArgs A)
{
    __shared__ uint32_t sh_lut[256];
    __shared__ int sh_front[4], sh_scan[4];
    __shared__ uint32_t sh_stage[kStage ? (kChunk * kVertexBytes + 3) / 4 + 1 : 1];
    const int tid = threadIdx.x, img = blockIdx.y, H = A.H, W = A.W, HW = H * W;
    sh_lut[tid] = (uint32_t)A.lut[tid * 3] | (uint32_t)A.lut[tid * 3 + 1] << 8 | (uint32_t)A.lut[tid * 3 + 2] << 16 | (uint32_t)A.alpha[tid] << 24;
    const int p0 = ((int)blockIdx.x * 256 + tid) * 4;
    const size_t cbase = (size_t)img * 3 * HW, pbase = (size_t)img * HW;
    const int front = chunks_in_front(A.chunks, A.C, 0, sh_front);

    int mask = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p0 + k < HW && valid_pt(cloud_at(A.c, cbase, p0 + k))) mask |= 1 << k;
    int total;
    const int excl = block_excl_scan<4>(__popc(mask), sh_scan, total);     // (its barrier also publishes sh_lut)

    // chunks is an input: whatever it holds, no record leaves the image's slot (with mesh_count's table room >= total)
    const int room = front >= 0 && front <= HW ? HW - front : 0;
    uint8_t* g0 = A.vbuf + (pbase + (size_t)(room ? front : 0)) * kVertexBytes;          // the chunk's first record
    const int start = kStage ? (int)((uintptr_t)g0 & 3) : 0;
    uint8_t* base = kStage ? reinterpret_cast<uint8_t*>(sh_stage) + start : g0;

    const double lo = A.lohi[A.lohi_per_image ? 2 * img : 0], hi = A.lohi[A.lohi_per_image ? 2 * img + 1 : 1];
    const double dlh = hi - lo;
    int y = p0 / W, x = p0 - y * W, rel = excl;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int q = p0 + k;
        if (q < HW) {
            const bool ok = (mask >> k) & 1;
            A.vidx[pbase + q] = ok ? front + rel : -1;
            if (ok && rel < room) {
                const Pt p = cloud_at(A.c, cbase, q);
                const Pt nw = pt_at(A.c, cbase, y - 1, x - 1, H, W), no = pt_at(A.c, cbase, y - 1, x, H, W);
                const Pt we = pt_at(A.c, cbase, y, x - 1, H, W), ea = pt_at(A.c, cbase, y, x + 1, H, W);
                const Pt so = pt_at(A.c, cbase, y + 1, x, H, W), se = pt_at(A.c, cbase, y + 1, x + 1, H, W);
                double nx = 0.0, ny = 0.0, nz = 0.0;
                tri_add(nw, no, p, A.max2, nx, ny, nz);      // cell (y-1, x-1) T0
                tri_add(nw, p, we, A.max2, nx, ny, nz);      // cell (y-1, x-1) T1
                tri_add(no, ea, p, A.max2, nx, ny, nz);      // cell (y-1, x)   T1
                tri_add(we, p, so, A.max2, nx, ny, nz);      // cell (y, x-1)   T0
                tri_add(p, ea, se, A.max2, nx, ny, nz);      // cell (y, x)     T0
                tri_add(p, se, so, A.max2, nx, ny, nz);      // cell (y, x)     T1
                const double len = sqrt((nx * nx + ny * ny) + nz * nz);
                float fx = 0.f, fy = 0.f, fz = 0.f;
                if (len > 0.0 && len < (double)INFINITY) fx = (float)(nx / len), fy = (float)(ny / len), fz = (float)(nz / len);
                if (A.flip) fx = -fx, fy = -fy, fz = -fz;

                const double s = A.maps[pbase + q];
                bool nan;
                const uint32_t e = sh_lut[overlay_index(s, lo, dlh, nan) & 255];
                uint32_t c = e & 0xffffffu;
                if (A.bg_kind == kBgU8) {
                    const uint8_t* __restrict__ b = (const uint8_t*)A.bg + (pbase + q) * 3;
                    c = blend_rgb(e, (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16);
                } else if (A.bg_kind == kBgF32) {
                    const float* __restrict__ b = (const float*)A.bg + cbase + q;
                    c = blend_rgb(e, bg_byte(b[0], A.mean[0], A.stdv[0]) | bg_byte(b[HW], A.mean[1], A.stdv[1]) << 8 |
                                         bg_byte(b[2 * (size_t)HW], A.mean[2], A.stdv[2]) << 16);
                }
                uint8_t* d = base + (size_t)rel * kVertexBytes;
                put32(d + 0, __float_as_uint(p.x)), put32(d + 4, __float_as_uint(p.y)), put32(d + 8, __float_as_uint(p.z));
                put32(d + 12, __float_as_uint(fx)), put32(d + 16, __float_as_uint(fy)), put32(d + 20, __float_as_uint(fz));
                d[24] = (uint8_t)c, d[25] = (uint8_t)(c >> 8), d[26] = (uint8_t)(c >> 16);
                put32(d + 27, __float_as_uint((float)s));
                put32(d + 31, A.labels ? (uint32_t)A.labels[pbase + q] : 0u);
            }
            rel += ok;
        }
        if (++x == W) x = 0, ++y;
    }
    if (kStage) {
        __syncthreads();
        flush_staged(sh_stage, g0, start, min(total, room) * kVertexBytes);
    }
}

template <bool kStage>
__global__ __launch_bounds__(256) void mesh_face_kernel(MeshArgs A)
{
    __shared__ int sh_front[4], sh_scan[4];
    __shared__ uint32_t sh_stage[kStage ? (2 * kChunk * kFaceBytes + 3) / 4 + 1 : 1];
    const int tid = threadIdx.x, img = blockIdx.y, H = A.H, W = A.W, HW = H * W;
    const int p0 = ((int)blockIdx.x * 256 + tid) * 4;
    const size_t cbase = (size_t)img * 3 * HW, pbase = (size_t)img * HW;
    const int front = chunks_in_front(A.chunks, A.C, 1, sh_front);

    int mask = 0;      // two bits per pixel
    {
        int y = p0 / W, x = p0 - y * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (p0 + k < HW) mask |= cell_faces(A.c, cbase, y, x, H, W, A.max2) << (2 * k);
            if (++x == W) x = 0, ++y;
        }
    }
    int total;
    const int excl = block_excl_scan<4>(__popc(mask), sh_scan, total);

    const int cap = 2 * (H - 1) * (W - 1);
    const int room = front >= 0 && front <= cap ? cap - front : 0;      // as in mesh_vertex_kernel
    uint8_t* g0 = A.fbuf + ((size_t)img * cap + (size_t)(room ? front : 0)) * kFaceBytes;
    const int start = kStage ? (int)((uintptr_t)g0 & 3) : 0;
    uint8_t* base = kStage ? reinterpret_cast<uint8_t*>(sh_stage) + start : g0;
    const int32_t* __restrict__ vi = A.vidx + pbase;
    int rel = excl;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int q = p0 + k, two = (mask >> (2 * k)) & 3;
        if (two) {
            const int ia = vi[q], ic = vi[q + W + 1];
            if ((two & 1) && rel < room) {
                const int ib = vi[q + 1];
                uint8_t* d = base + (size_t)rel * kFaceBytes;
                d[0] = 3;
                put32(d + 1, (uint32_t)ia), put32(d + 5, (uint32_t)(A.flip ? ic : ib)), put32(d + 9, (uint32_t)(A.flip ? ib : ic));
            }
            rel += two & 1;
            if ((two & 2) && rel < room) {
                const int id = vi[q + W];
                uint8_t* d = base + (size_t)rel * kFaceBytes;
                d[0] = 3;
                put32(d + 1, (uint32_t)ia), put32(d + 5, (uint32_t)(A.flip ? id : ic)), put32(d + 9, (uint32_t)(A.flip ? ic : id));
            }
            rel += two >> 1;
        }
    }
    if (kStage) {
        __syncthreads();
        flush_staged(sh_stage, g0, start, min(total, room) * kFaceBytes);
    }
}

bool geometry_ok(const char* who, int n, int H, int W, long long pix_stride, long long ch_stride, double max_edge2)
{
    if (!(side_ok(H) && side_ok(W) && n >= 0 && n <= kMaxImages && (long long)n * H * W <= kMeshMaxTotal)) {
        cmdiad_set_error("%s: bad sizes n=%d (0..%d) H=%d W=%d (sides 1..%d, n*H*W <= %d)", who, n, kMaxImages, H, W, kMaxSide, kMeshMaxTotal);
        return false;
    }
    const long long HW = (long long)H * W;
    if (!cloud_strides_ok(pix_stride, ch_stride, HW)) {
        cmdiad_set_error("%s: bad strides pix_stride=%lld ch_stride=%lld (planar [n,3,H,W]: 1 and H*W = %lld; interleaved [n,H,W,3]: 3 "
                         "and 1)", who, pix_stride, ch_stride, HW);
        return false;
    }
    if (!(max_edge2 > 0.0)) {      // (a NaN fails the comparison; +inf passes: no cut)
        cmdiad_set_error("%s: max_edge2=%g must be > 0 (+inf: no edge is cut)", who, max_edge2);
        return false;
    }
    return true;
}

template <bool kStage>
int launch_write(const MeshArgs& A, int n, bool cells, hipStream_t s)
{
    const dim3 grid((unsigned)A.C, (unsigned)n);
    hipLaunchKernelGGL(mesh_vertex_kernel<kStage>, grid, dim3(256), 0, s, A);
    CMDIAD_CHECK_LAUNCH();
    if (!cells) return CMDIAD_OK;      // a single row or column has no cell: no face, no launch
    hipLaunchKernelGGL(mesh_face_kernel<kStage>, grid, dim3(256), 0, s, A);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

}  // namespace

extern "C" int cmdiad_mesh_count(const float* cloud, long long pix_stride, long long ch_stride, const double* maps, int n, int H, int W,
                                 double max_edge2, int32_t* chunks, int32_t* counts, cmdiad_stream_t stream)
{
    if (!geometry_ok("cmdiad_mesh_count", n, H, W, pix_stride, ch_stride, max_edge2)) return CMDIAD_ERR_ARG;
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(cloud && maps && chunks && counts, CMDIAD_ERR_ARG, "cmdiad_mesh_count: null pointer (cloud, maps, chunks, counts)");
    hipStream_t s = (hipStream_t)stream;
    CMDIAD_CHECK_HIP("cmdiad_mesh_count", hipMemsetAsync(counts, 0, (size_t)n * 4 * sizeof(int32_t), s));
    const int C = (H * W + kChunk - 1) / kChunk;
    const Cloud c = {cloud, pix_stride, ch_stride};
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)C, (unsigned)n), dim3(256), 0, s, c, maps, H, W, C, max_edge2, chunks, counts);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_mesh_write(const float* cloud, long long pix_stride, long long ch_stride, const double* maps, int n, int H, int W,
                                 const double* lohi, int lohi_per_image, const uint8_t* lut, const uint8_t* alpha, const void* bg,
                                 int bg_kind, double mean_r, double mean_g, double mean_b, double std_r, double std_g, double std_b,
                                 const int32_t* labels, double max_edge2, int flip, const int32_t* chunks, int32_t* vidx,
                                 uint8_t* vertices, uint8_t* faces, cmdiad_stream_t stream)
{
    if (!geometry_ok("cmdiad_mesh_write", n, H, W, pix_stride, ch_stride, max_edge2)) return CMDIAD_ERR_ARG;
    CMDIAD_REQUIRE((lohi_per_image == 0 || lohi_per_image == 1) && (flip == 0 || flip == 1), CMDIAD_ERR_ARG,
                   "cmdiad_mesh_write: lohi_per_image=%d flip=%d (0 | 1)", lohi_per_image, flip);
    CMDIAD_REQUIRE(bg_kind == kBgNone || bg_kind == kBgU8 || bg_kind == kBgF32, CMDIAD_ERR_ARG,
                   "cmdiad_mesh_write: background kind %d (0 none | 1 uint8 [n,H,W,3] | 2 float32 [n,3,H,W])", bg_kind);
    if (n == 0) return CMDIAD_OK;
    const bool cells = H > 1 && W > 1;
    CMDIAD_REQUIRE(cloud && maps && lohi && lut && alpha && chunks && vidx && vertices && (faces || !cells) && (bg_kind == kBgNone || bg),
                   CMDIAD_ERR_ARG, "cmdiad_mesh_write: null pointer (cloud, maps, lohi, lut, alpha, chunks, vidx, vertices; faces where "
                   "H and W are above 1; bg with a background kind)");
    MeshArgs A;
    A.c = {cloud, pix_stride, ch_stride};
    A.maps = maps, A.lohi = lohi, A.bg = bg, A.lut = lut, A.alpha = alpha, A.labels = labels, A.chunks = chunks;
    A.vidx = vidx, A.vbuf = vertices, A.fbuf = faces, A.max2 = max_edge2;
    A.mean[0] = mean_r, A.mean[1] = mean_g, A.mean[2] = mean_b, A.stdv[0] = std_r, A.stdv[1] = std_g, A.stdv[2] = std_b;
    A.H = H, A.W = W, A.C = (H * W + kChunk - 1) / kChunk;
    A.lohi_per_image = lohi_per_image, A.bg_kind = bg_kind, A.flip = flip;
    hipStream_t s = (hipStream_t)stream;
#ifdef CMDIAD_AB_VARIANTS
    // the test-only build carries both store variants: CMDIAD_MESH_STORE = 'l...' (staged in LDS) | 'b...' (byte stores)
    if (env_set("CMDIAD_MESH_STORE")) return env_is("CMDIAD_MESH_STORE", 'l') ? launch_write<true>(A, n, cells, s) : launch_write<false>(A, n, cells, s);
#endif
    return launch_write<kStageDefault>(A, n, cells, s);
}
