// mesh.hip -- mesh extraction for gfx950 (no reference counterpart): bounded TSDF fusion of depth maps into a dense volume, and
// welded marching tetrahedra over it. Compiled without contraction: every fp32 operation below is rounded on its own, in the
// order written, and tests/mesh_ref.py repeats them in NumPy bit for bit.
//
// THE VOLUME. Nx x Ny x Nz lattice points at origin + (i, j, k) h, each component formed as origin + float(index) * h; fp32 planes
// [Nz, Ny, Nx] (x fastest, linear index (k Ny + j) Nx + i): tsdf, weight and, optionally, three colour planes behind one pointer.
// N = Nx Ny Nz <= 2^31 - 1.
//
// INTEGRATE (tsdf_integrate_kernel). One lane per lattice point, a wave covers 64 consecutive x: the five plane values are loaded
// once (coalesced), kept in registers over the K cameras of the table (filter3d.hip's 16-float rows; the camera index is the loop
// counter and the table a const restrict argument, so the rows arrive by scalar loads), and stored once, only where a camera
// updated the point. For camera c, in table order, with p the point:
//     x = ((m0 px + m1 py) + m2 pz) + m3, y and z likewise                       (filter3d.hip's expression)
//     skip if z < depth_min
//     u = (fx x) / z + 0.5 W,  v = (fy y) / z + 0.5 H;   skip unless 0 <= u < W and 0 <= v < H
//     d = depth[c][int(v)][int(u)];                      skip unless 0 < d <= depth_max   (a NaN depth is skipped)
//     sdf = d - z;                                       skip if sdf < -sdf_trunc
//     s = min(1, sdf / sdf_trunc);  tsdf = (tsdf w + s) / (w + 1), every colour plane likewise with the pixel's colour;  w = w + 1
// No atomics: a point has one owner. The depth gather is the only irregular access; neighbouring points project to neighbouring
// pixels, so it is served by L2. Bounds: the volume is read and written once per launch (20 B per point each way with colours);
// per camera a lane spends about 40 VALU operations and three correctly rounded divisions, so from a handful of cameras on the
// launch is bound by the vector ALU, not by HBM.
//
// EXTRACT. A cell is cut into the six Kuhn tetrahedra around its main diagonal: the paths (0,0,0) -> +a -> +a+b -> (1,1,1) for the
// permutations (a, b, c) of the axes in lexicographic order (x < y < z). Every tetrahedron edge points in a non-negative
// direction, so the lattice edge between a < b is owned by a in one of 7 slots: +x, +y, +z, +xy, +xz, +yz, +xyz. A corner is inside
// iff its value is < 0. A vertex exists on an edge iff its endpoints differ in sign and a cell whose eight corners all have
// weight > 0 contains the edge; it lies at pa + t (pb - pa), t = va / (va - vb), colours likewise.
//   mesh_classify_kernel   one lane per point: the 27 weights around it give the validity of the 7 cells that contain its edges, the
//                          8 values at and above it the signs -> one byte per point (bits 0..6 the edge slots, bit 7: its own cell
//                          is valid) and the per-block totals of vertices and triangles
//   mesh_scan_kernel       scan_blocks.hpp over both total arrays; the two grand totals go to one 8-byte slot, the host's one read
//   mesh_vertices_kernel   one lane per point: its vertex base (block base + scan of the block's popcounts) -> base[point], and its
//                          vertices; an edge's vertex index is base[owner] + popcount(mask[owner] & below(slot)) -- 5 bytes a point
//   mesh_faces_kernel      one lane per cell: triangles of its six tetrahedra behind block base + in-block scan of the counts
// Triangles, with path positions of the inside corners (a, b) and outside corners (c, d) ascending: one inside a: (a o1, a o2,
// a o3); three inside: the same about the outside corner; two inside: (ac, ad, bd) and (ac, bd, bc). Winding is combinatorial (the
// parity of the corner order against the tetrahedron's orientation), so zero-area triangles are wound like their neighbours:
// the normal points from the negative to the positive side.
// Vertex and face totals are 32-bit; the emit kernels refuse to store past the counts they are given.
#include "common.hpp"
#include "scan_blocks.hpp"

namespace c3dgs {

namespace {

constexpr int MESH_BLOCK = 256;

template <bool COLOR>
__global__ void __launch_bounds__(MESH_BLOCK) tsdf_integrate_kernel(const c3dgs_lattice g, const uint32_t N, const int K, const int W,
                                                                    const int H, const float* __restrict__ depth,
                                                                    const float* __restrict__ color,
                                                                    const float* __restrict__ cams, const float trunc,
                                                                    const float depth_min, const float depth_max,
                                                                    float* __restrict__ tsdf, float* __restrict__ weight,
                                                                    float* __restrict__ vcol)
{
    const uint32_t idx = blockIdx.x * (uint32_t)MESH_BLOCK + threadIdx.x;
    if (idx >= N) return;
    const uint32_t i = idx % (uint32_t)g.Nx, r = idx / (uint32_t)g.Nx, j = r % (uint32_t)g.Ny, k = r / (uint32_t)g.Ny;
    const float px = g.ox + (float)i * g.voxel_size, py = g.oy + (float)j * g.voxel_size, pz = g.oz + (float)k * g.voxel_size;
    float t = tsdf[idx], w = weight[idx], c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (COLOR) { c0 = vcol[idx]; c1 = vcol[(size_t)N + idx]; c2 = vcol[2 * (size_t)N + idx]; }
    const size_t plane = (size_t)W * (size_t)H;
    bool touched = false;
    for (int c = 0; c < K; c++) {
        const float* __restrict__ m = cams + 16 * (size_t)c;
        const float x = m[0] * px + m[1] * py + m[2] * pz + m[3];
        const float y = m[4] * px + m[5] * py + m[6] * pz + m[7];
        const float z = m[8] * px + m[9] * py + m[10] * pz + m[11];
        if (z < depth_min) continue;
        const float fx = m[12], fy = m[13], Wf = m[14], Hf = m[15];
        const float u = fx * x / z + 0.5f * Wf;
        const float v = fy * y / z + 0.5f * Hf;
        if (!(u >= 0.f && u < Wf && v >= 0.f && v < Hf)) continue;
        const int ui = (int)u, vi = (int)v;
        if (ui >= W || vi >= H) continue;                  // a table whose W, H are not the maps': never outside the maps
        const size_t pix = (size_t)vi * (size_t)W + (size_t)ui;
        const float d = depth[(size_t)c * plane + pix];
        if (!(d > 0.f) || d > depth_max) continue;
        const float sdf = d - z;
        if (sdf < -trunc) continue;
        const float s = fminf(1.f, sdf / trunc);
        const float w1 = w + 1.f;
        t = (t * w + s) / w1;
        if (COLOR) {
            const float* __restrict__ cp = color + 3 * (size_t)c * plane + pix;
            c0 = (c0 * w + cp[0]) / w1;
            c1 = (c1 * w + cp[plane]) / w1;
            c2 = (c2 * w + cp[2 * plane]) / w1;
        }
        w = w1;
        touched = true;
    }
    if (!touched) return;
    tsdf[idx] = t; weight[idx] = w;
    if (COLOR) { vcol[idx] = c0; vcol[(size_t)N + idx] = c1; vcol[2 * (size_t)N + idx] = c2; }
}

// ---- marching tetrahedra
// cell-local corner codes: bit 0 = +x, bit 1 = +y, bit 2 = +z. The six Kuhn paths, by permutation in lexicographic order, and
// whether the path's orientation det[q1 - q0, q2 - q0, q3 - q0] is negative (an odd permutation).
__device__ constexpr uint8_t TET_CORNER[6][4] = { { 0, 1, 3, 7 }, { 0, 1, 5, 7 }, { 0, 2, 3, 7 }, { 0, 2, 6, 7 }, { 0, 4, 5, 7 },
                                                  { 0, 4, 6, 7 } };
__device__ constexpr uint8_t TET_ODD[6] = { 0, 1, 1, 0, 0, 1 };
// direction code (the xor of an edge's two corner codes) -> slot: +x, +y, +z, +xy, +xz, +yz, +xyz
__device__ constexpr uint8_t DIR_SLOT[8] = { 0, 0, 1, 3, 2, 4, 5, 6 };
__device__ constexpr uint8_t SLOT_DIR[7] = { 1, 2, 4, 3, 5, 6, 7 };

__device__ __forceinline__ int tet_inside(const uint32_t signs, const int t)
{
    int m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) m |= (int)((signs >> TET_CORNER[t][q]) & 1u) << q;
    return m;
}

__device__ __forceinline__ int cell_triangles(const uint32_t signs)
{
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const int c = __popc(tet_inside(signs, t));
        n += c == 2 ? 2 : ((c == 1 || c == 3) ? 1 : 0);
    }
    return n;
}

// exclusive scan of `v` over the block's 256 threads (all must call) -> the thread's base; `total`: the block's sum
__device__ __forceinline__ uint32_t block_exclusive(const uint32_t v, uint32_t& total)
{
    __shared__ uint32_t s_w[MESH_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    __syncthreads();                                       // a second call: the previous one's readers are done
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t off = 0; total = 0;
#pragma unroll
    for (int q = 0; q < MESH_BLOCK / 64; q++) { const uint32_t x = s_w[q]; if (q < wave) off += x; total += x; }
    return off + incl - v;
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_classify_kernel(const c3dgs_lattice g, const uint32_t N,
                                                                   const float* __restrict__ tsdf,
                                                                   const float* __restrict__ weight, uint8_t* __restrict__ mask,
                                                                   uint32_t* __restrict__ block_v, uint32_t* __restrict__ block_t)
{
    const uint32_t idx = blockIdx.x * (uint32_t)MESH_BLOCK + threadIdx.x;
    uint32_t nv = 0, nt = 0;
    if (idx < N) {
        const int i = (int)(idx % (uint32_t)g.Nx), r = (int)(idx / (uint32_t)g.Nx), j = r % g.Ny, k = r / g.Ny;
        const size_t sy = (size_t)g.Nx, sz = (size_t)g.Nx * (size_t)g.Ny;
        // bit (dz+1) 9 + (dy+1) 3 + (dx+1): that neighbour is in the lattice and has weight > 0
        uint32_t wb = 0;
        // every cell that contains one of the point's edges has the point as a corner: without its own weight nothing to look at
        if (weight[idx] > 0.f) {
#pragma unroll
            for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const int x = i + dx, y = j + dy, z = k + dz;
                        if (x < 0 || y < 0 || z < 0 || x >= g.Nx || y >= g.Ny || z >= g.Nz) continue;
                        if (weight[(size_t)z * sz + (size_t)y * sy + (size_t)x] > 0.f)
                            wb |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
                    }
        }
        // bit (cz+1) 4 + (cy+1) 2 + (cx+1), c in {-1, 0}^3: the cell whose low corner is point + c has eight weighted corners
        uint32_t cells = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            uint32_t need = 0;
#pragma unroll
            for (int q = 0; q < 8; q++)
                need |= 1u << (((c >> 2) + (q >> 2)) * 9 + (((c >> 1) & 1) + ((q >> 1) & 1)) * 3 + ((c & 1) + (q & 1)));
            if ((wb & need) == need) cells |= 1u << c;
        }
        uint32_t m = 0;
        if (cells) {
            // the signs of the point and of the seven above it (the corners of its own cell); outside the lattice: no valid cell
            // contains the edge, whatever the bit says
            uint32_t signs = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int x = i + (q & 1), y = j + ((q >> 1) & 1), z = k + (q >> 2);
                if (x >= g.Nx || y >= g.Ny || z >= g.Nz) continue;
                if (tsdf[(size_t)z * sz + (size_t)y * sy + (size_t)x] < 0.f) signs |= 1u << q;
            }
#pragma unroll
            for (int s = 0; s < 7; s++) {
                const int d = SLOT_DIR[s];
                if ((((signs >> d) ^ signs) & 1u) == 0) continue;
                // the cells that contain the edge: offset 0 along the edge's axes, -1 or 0 along the others
                uint32_t around = 0;
#pragma unroll
                for (int c = 0; c < 8; c++)
                    if (((~c & 7) & d) == 0) around |= 1u << c;       // c has bit a set <=> offset 0 along a
                if (cells & around) m |= 1u << s;
            }
            if (cells & 0x80u) { m |= 0x80u; nt = (uint32_t)cell_triangles(signs); }
            nv = (uint32_t)__popc(m & 0x7fu);
        }
        mask[idx] = (uint8_t)m;
    }
    uint32_t tv, tt;
    block_exclusive(nv, tv);
    block_exclusive(nt, tt);
    if (threadIdx.x == 0) { block_v[blockIdx.x] = tv; block_t[blockIdx.x] = tt; }
}

__global__ void __launch_bounds__(SCAN_BLOCKS_THREADS) mesh_scan_kernel(const int nb, uint32_t* __restrict__ block_v,
                                                                        uint32_t* __restrict__ block_t,
                                                                        uint32_t* __restrict__ totals)
{
    scan_blocks_body(nb, block_v, nullptr, nullptr, 0u);
    __syncthreads();
    scan_blocks_body(nb, block_t, nullptr, nullptr, 0u);
    if (threadIdx.x == 0) { totals[0] = block_v[nb]; totals[1] = block_t[nb]; }
}

template <bool COLOR>
__global__ void __launch_bounds__(MESH_BLOCK) mesh_vertices_kernel(const c3dgs_lattice g, const uint32_t N, const uint32_t V,
                                                                   const float* __restrict__ tsdf, const float* __restrict__ vcol,
                                                                   const uint8_t* __restrict__ mask,
                                                                   const uint32_t* __restrict__ block_v, uint32_t* __restrict__ base,
                                                                   float* __restrict__ vertices, float* __restrict__ colors)
{
    const uint32_t idx = blockIdx.x * (uint32_t)MESH_BLOCK + threadIdx.x;
    const uint32_t m = idx < N ? (uint32_t)mask[idx] & 0x7fu : 0u;
    uint32_t total;
    uint32_t at = block_v[blockIdx.x] + block_exclusive((uint32_t)__popc(m), total);
    if (idx >= N) return;
    base[idx] = at;
    if (!m) return;
    const int i = (int)(idx % (uint32_t)g.Nx), r = (int)(idx / (uint32_t)g.Nx), j = r % g.Ny, k = r / g.Ny;
    const size_t sy = (size_t)g.Nx, sz = (size_t)g.Nx * (size_t)g.Ny;
    const float pa[3] = { g.ox + (float)i * g.voxel_size, g.oy + (float)j * g.voxel_size, g.oz + (float)k * g.voxel_size };
    const float va = tsdf[idx];
    float ca[3] = { 0.f, 0.f, 0.f };
    if (COLOR) { ca[0] = vcol[idx]; ca[1] = vcol[(size_t)N + idx]; ca[2] = vcol[2 * (size_t)N + idx]; }
    for (int s = 0; s < 7; s++) {
        if (!((m >> s) & 1u)) continue;
        const int d = SLOT_DIR[s];
        const int x = i + (d & 1), y = j + ((d >> 1) & 1), z = k + (d >> 2);       // inside the lattice: a valid cell holds the edge
        if (x >= g.Nx || y >= g.Ny || z >= g.Nz) continue;                         // (a workspace that is not the count's)
        const size_t b = (size_t)z * sz + (size_t)y * sy + (size_t)x;
        const float vb = tsdf[b];
        const float t = va / (va - vb);
        const float pb[3] = { g.ox + (float)x * g.voxel_size, g.oy + (float)y * g.voxel_size, g.oz + (float)z * g.voxel_size };
        if (at < V) {
#pragma unroll
            for (int q = 0; q < 3; q++) vertices[3 * (size_t)at + q] = pa[q] + t * (pb[q] - pa[q]);
            if (COLOR) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const float cb = vcol[(size_t)q * N + b];
                    colors[3 * (size_t)at + q] = ca[q] + t * (cb - ca[q]);
                }
            }
        }
        at++;
    }
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_faces_kernel(const c3dgs_lattice g, const uint32_t N, const uint32_t F,
                                                                const float* __restrict__ tsdf, const uint8_t* __restrict__ mask,
                                                                const uint32_t* __restrict__ block_t,
                                                                const uint32_t* __restrict__ base, int32_t* __restrict__ faces)
{
    const uint32_t idx = blockIdx.x * (uint32_t)MESH_BLOCK + threadIdx.x;
    bool cell = idx < N && (mask[idx] & 0x80u);
    uint32_t signs = 0;
    int i = 0, j = 0, k = 0;
    const size_t sy = (size_t)g.Nx, sz = (size_t)g.Nx * (size_t)g.Ny;
    if (cell) {                                             // a valid cell: its eight corners are inside the lattice
        i = (int)(idx % (uint32_t)g.Nx); const int r = (int)(idx / (uint32_t)g.Nx); j = r % g.Ny; k = r / g.Ny;
        cell = i + 1 < g.Nx && j + 1 < g.Ny && k + 1 < g.Nz;                       // (a workspace that is not the count's)
    }
    if (cell) {
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (tsdf[(size_t)(k + (q >> 2)) * sz + (size_t)(j + ((q >> 1) & 1)) * sy + (size_t)(i + (q & 1))] < 0.f) signs |= 1u << q;
    }
    const uint32_t nt = cell ? (uint32_t)cell_triangles(signs) : 0u;
    uint32_t total;
    uint32_t at = block_t[blockIdx.x] + block_exclusive(nt, total);
    if (!nt) return;
    // the vertex base and edge mask of the seven corners that own edges of this cell
    uint32_t cbase[7], cmask[7];
#pragma unroll
    for (int q = 0; q < 7; q++) {
        const size_t p = (size_t)(k + (q >> 2)) * sz + (size_t)(j + ((q >> 1) & 1)) * sy + (size_t)(i + (q & 1));
        cbase[q] = base[p]; cmask[q] = mask[p];
    }
    for (int t = 0; t < 6; t++) {
        const int in = tet_inside(signs, t), n = __popc(in);
        if (n == 0 || n == 4) continue;
        // L: path positions, for one or two inside corners the inside ones first, for three the outside one first
        const int first = n == 3 ? (~in & 15) : in;
        int L[4], nl = 0;
        for (int q = 0; q < 4; q++) if ((first >> q) & 1) L[nl++] = q;
        for (int q = 0; q < 4; q++) if (!((first >> q) & 1)) L[nl++] = q;
        int inv = 0;
        for (int a = 0; a < 4; a++) for (int b = a + 1; b < 4; b++) inv += L[a] > L[b];
        // orientation of the corners in L's order: the path's, times the parity of L
        const bool positive = ((inv & 1) ^ TET_ODD[t]) == 0;
        const bool keep = n == 3 ? !positive : positive;
        auto vertex = [&](const int p, const int q) -> int32_t {
            const int lo = TET_CORNER[t][p < q ? p : q], hi = TET_CORNER[t][p < q ? q : p];
            const int s = DIR_SLOT[lo ^ hi];
            uint32_t b = 0, mk = 0;
#pragma unroll
            for (int c = 0; c < 7; c++) if (c == lo) { b = cbase[c]; mk = cmask[c]; }
            return (int32_t)(b + (uint32_t)__popc(mk & ((1u << s) - 1u)));
        };
        int32_t tri[2][3];
        if (n == 2) {
            const int32_t ac = vertex(L[0], L[2]), ad = vertex(L[0], L[3]), bd = vertex(L[1], L[3]), bc = vertex(L[1], L[2]);
            tri[0][0] = ac; tri[0][1] = ad; tri[0][2] = bd;
            tri[1][0] = ac; tri[1][1] = bd; tri[1][2] = bc;
        } else {
            tri[0][0] = vertex(L[0], L[1]); tri[0][1] = vertex(L[0], L[2]); tri[0][2] = vertex(L[0], L[3]);
        }
        for (int q = 0; q < (n == 2 ? 2 : 1); q++, at++) {
            if (at >= F) continue;
            faces[3 * (size_t)at] = tri[q][0];
            faces[3 * (size_t)at + 1] = keep ? tri[q][1] : tri[q][2];
            faces[3 * (size_t)at + 2] = keep ? tri[q][2] : tri[q][1];
        }
    }
}

inline uint32_t mesh_blocks(const uint32_t N) { return (N + MESH_BLOCK - 1) / MESH_BLOCK; }
inline size_t up256(const size_t v) { return (v + 255) & ~(size_t)255; }

struct MeshWs { uint8_t* mask; uint32_t* base; uint32_t* block_v; uint32_t* block_t; uint32_t* totals; size_t bytes; };

// [mask: a byte per point][base: a word per point][block_v, block_t: a word per block, scan_blocks.hpp's slack][totals]
MeshWs mesh_ws(void* ws, const uint32_t N)
{
    const size_t nb = mesh_blocks(N);
    const size_t totals_at = ((nb + 2 + 15) & ~(size_t)15) * sizeof(uint32_t);
    uint8_t* p = (uint8_t*)ws;
    MeshWs w;
    size_t at = 0;
    w.mask = p + at; at += up256(N);
    w.base = (uint32_t*)(p + at); at += up256((size_t)N * 4);
    w.block_v = (uint32_t*)(p + at); at += up256(totals_at);
    w.block_t = (uint32_t*)(p + at); at += up256(totals_at);
    w.totals = (uint32_t*)(p + at); at += 256;
    w.bytes = at;
    return w;
}

} // namespace

void launch_tsdf_integrate(const c3dgs_lattice& l, int K, int W, int H, const float* depth, const float* color, const float* cams,
                           float sdf_trunc, float depth_min, float depth_max, float* tsdf, float* weight, float* vol_color,
                           hipStream_t s)
{
    const uint32_t N = (uint32_t)((size_t)l.Nx * l.Ny * l.Nz);
    if (color) tsdf_integrate_kernel<true><<<mesh_blocks(N), MESH_BLOCK, 0, s>>>(l, N, K, W, H, depth, color, cams, sdf_trunc, depth_min,
                                                                                depth_max, tsdf, weight, vol_color);
    else tsdf_integrate_kernel<false><<<mesh_blocks(N), MESH_BLOCK, 0, s>>>(l, N, K, W, H, depth, nullptr, cams, sdf_trunc, depth_min,
                                                                           depth_max, tsdf, weight, nullptr);
}

size_t mesh_extract_workspace_bytes(int Nx, int Ny, int Nz) { return mesh_ws(nullptr, (uint32_t)((size_t)Nx * Ny * Nz)).bytes; }

void launch_mesh_classify(const c3dgs_lattice& l, const float* tsdf, const float* weight, void* ws, hipStream_t s)
{
    const uint32_t N = (uint32_t)((size_t)l.Nx * l.Ny * l.Nz);
    const MeshWs w = mesh_ws(ws, N);
    mesh_classify_kernel<<<mesh_blocks(N), MESH_BLOCK, 0, s>>>(l, N, tsdf, weight, w.mask, w.block_v, w.block_t);
}

const uint32_t* launch_mesh_scan(const c3dgs_lattice& l, void* ws, hipStream_t s)
{
    const uint32_t N = (uint32_t)((size_t)l.Nx * l.Ny * l.Nz);
    const MeshWs w = mesh_ws(ws, N);
    mesh_scan_kernel<<<1, SCAN_BLOCKS_THREADS, 0, s>>>((int)mesh_blocks(N), w.block_v, w.block_t, w.totals);
    return w.totals;
}

void launch_mesh_vertices(const c3dgs_lattice& l, const float* tsdf, const float* vol_color, void* ws, uint32_t V, float* vertices,
                          float* colors, hipStream_t s)
{
    const uint32_t N = (uint32_t)((size_t)l.Nx * l.Ny * l.Nz);
    const MeshWs w = mesh_ws(ws, N);
    if (vol_color) mesh_vertices_kernel<true><<<mesh_blocks(N), MESH_BLOCK, 0, s>>>(l, N, V, tsdf, vol_color, w.mask, w.block_v, w.base,
                                                                                   vertices, colors);
    else mesh_vertices_kernel<false><<<mesh_blocks(N), MESH_BLOCK, 0, s>>>(l, N, V, tsdf, nullptr, w.mask, w.block_v, w.base, vertices,
                                                                          nullptr);
}

void launch_mesh_faces(const c3dgs_lattice& l, const float* tsdf, void* ws, uint32_t F, int32_t* faces, hipStream_t s)
{
    const uint32_t N = (uint32_t)((size_t)l.Nx * l.Ny * l.Nz);
    const MeshWs w = mesh_ws(ws, N);
    mesh_faces_kernel<<<mesh_blocks(N), MESH_BLOCK, 0, s>>>(l, N, F, tsdf, w.mask, w.block_t, w.base, faces);
}

} // namespace c3dgs
