// k_mesh.hip -- the triangle mesh of a disparity map (include/adcensus_c_api.h: adc_mesh_device; the cell rule is mesh_cell.h): a
// stencil over the lattice of every step-th pixel and two ordered compactions, in the shape of k_outputs.hip.  The lattice is walked
// in raster-linear chunks of 64 lattice points, one chunk per wave and turn, so a chunk may wrap lattice rows.
//
// Three launches on the object stream, none of which depends on another workgroup of its own launch:
//   k_mesh_measure  per lattice point the code of the cell whose corner A it is (a byte map, written only when triangles are asked
//                   for) and its "used" bit from the codes of the four cells around it -- the three neighbouring codes are recomputed
//                   from the map's values (a 3 x 3 neighbourhood per lane), never read from the byte map; per chunk the 64-bit ballot
//                   of "used", the count of used points and the count of triangles; per workgroup one integer atomic per report count
//   k_mesh_scan     one workgroup: exclusive scans of the two per-chunk count arrays in place, side by side, the totals -> the report words and
//                   the caller's two count words
//   k_mesh_emit     vertices behind their chunk's base at the rank v_mbcnt gives, with vertex_index; triangles behind their chunk's
//                   base, a corner's vertex number = vertex base + popcount(used word & lanes below) of the corner's OWN chunk
// Every count is an integer and every rank a prefix of a ballot: the result does not depend on the order in which waves run.
#include "adc_internal.h"
#include "mesh_cell.h"

#define MESH_WG 256
#define MESH_WAVES (MESH_WG / ADC_WAVE)
#define MESH_PER_WAVE 4                               // chunks a wave owns
#define MESH_TILE (MESH_WG * MESH_PER_WAVE)           // lattice points per workgroup
#define MESH_REP_WORDS 8                              // adc_mesh_report

struct MeshArgs {
    const float* disp;
    const uint8_t* img;            // may be null
    MeshCam cam;
    float max_diff;
    int step, W, Wl, Hl, Nl;       // Nl = Wl * Hl lattice points
    uint32_t* rep;                 // [0] lattice_valid [1] vertices [2] triangles [3] cells_two [4] cells_one
    uint32_t* vbase;               // per chunk: used points -> (scan) vertices of all chunks before it
    uint32_t* tbase;               // per chunk: triangles -> (scan) triangles of all chunks before it
    unsigned long long* used;      // per chunk: ballot of "used"
    uint8_t* codes;                // per lattice point: the code of its cell; null when no triangles are asked for
    uint4* vertices;               // may be null
    int32_t* vindex;               // may be null
    uint32_t* triangles;           // may be null
    uint32_t vcap, tcap;
    uint32_t* counts;              // may be null
};

// a = fabsf(d) and the validity of lattice point (i, j); outside the lattice: invalid
__device__ __forceinline__ bool mesh_fetch(const MeshArgs& g, bool in, int i, int j, float* a)
{
    *a = ADC_INVALID_FLOAT;
    if (!in || i < 0 || i >= g.Wl || j < 0 || j >= g.Hl) return false;
    *a = __builtin_fabsf(g.disp[(size_t)(j * g.step) * (size_t)g.W + (size_t)(i * g.step)]);
    return mesh_valid(g.cam, *a);
}

__global__ __launch_bounds__(MESH_WG) void k_mesh_measure(const MeshArgs g)
{
    __shared__ uint32_t s_cnt[3][MESH_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    uint32_t n_valid = 0, n_two = 0, n_one = 0;
#pragma unroll 1
    for (int k = 0; k < MESH_PER_WAVE; k++) {
        const int chunk = ((int)blockIdx.x * MESH_WAVES + wave) * MESH_PER_WAVE + k;
        if (chunk * ADC_WAVE >= g.Nl) continue; // (uniform in the wave)
        const int L = chunk * ADC_WAVE + lane;
        const bool in = L < g.Nl;
        const int j = L / g.Wl, i = L - j * g.Wl;
        float a[3][3];
        bool v[3][3];
#pragma unroll
        for (int dj = 0; dj < 3; dj++)
#pragma unroll
            for (int di = 0; di < 3; di++) v[dj][di] = mesh_fetch(g, in, i + di - 1, j + dj - 1, &a[dj][di]);
        uint32_t code[2][2]; // code[dj][di]: the cell whose corner A is lattice (i + di - 1, j + dj - 1)
#pragma unroll
        for (int dj = 0; dj < 2; dj++)
#pragma unroll
            for (int di = 0; di < 2; di++) {
                const float ca[4] = {a[dj][di], a[dj][di + 1], a[dj + 1][di], a[dj + 1][di + 1]};
                const bool cv[4] = {v[dj][di], v[dj][di + 1], v[dj + 1][di], v[dj + 1][di + 1]};
                code[dj][di] = mesh_cell_code(ca, cv, g.max_diff);
            }
        const uint32_t own = code[1][1];
        const bool used = mesh_code_uses(own, MESH_A) || mesh_code_uses(code[1][0], MESH_B) || mesh_code_uses(code[0][1], MESH_C) || mesh_code_uses(code[0][0], MESH_D);
        if (g.codes && in) g.codes[L] = (uint8_t)own;
        const unsigned long long um = __ballot(used), t0 = __ballot((own & MESH_T0) != 0), t1 = __ballot((own & MESH_T1) != 0);
        if (lane == 0) {
            g.used[chunk] = um;
            g.vbase[chunk] = (uint32_t)__popcll(um);
            g.tbase[chunk] = (uint32_t)__popcll(t0) + (uint32_t)__popcll(t1);
        }
        n_valid += (uint32_t)__popcll(__ballot(v[1][1]));
        n_two += (uint32_t)__popcll(t0 & t1);
        n_one += (uint32_t)__popcll(t0 ^ t1);
    }
    if (lane == 0) { s_cnt[0][wave] = n_valid; s_cnt[1][wave] = n_two; s_cnt[2][wave] = n_one; }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t t = 0;
        for (int w = 0; w < MESH_WAVES; w++) t += s_cnt[threadIdx.x][w];
        if (t) atomicAdd(&g.rep[threadIdx.x == 0 ? 0 : 2 + threadIdx.x], t); // lattice_valid, cells_two, cells_one
    }
}

// One workgroup of 1024: both arrays of per-chunk counts -> exclusive prefix sums in place, MESH_SCAN_TILE entries of each at a time
// with a carry (the form of k_out_scan; a lane owns four consecutive entries of each array, so 1080p at step 1 -- 32400 chunks -- takes
// 8 turns; with the two arrays one after the other and one entry per lane it took 64 turns and 58 us, the longest launch of the call:
// profiles/mesh_timing.md); the totals go to the report
// words (read back by the launcher) and to the caller's device words.
#define MESH_SCAN_PER_LANE 4
#define MESH_SCAN_TILE (1024 * MESH_SCAN_PER_LANE)
__global__ __launch_bounds__(1024) void k_mesh_scan(uint32_t* __restrict__ vbase, uint32_t* __restrict__ tbase, int nchunks, uint32_t* __restrict__ rep,
                                                    uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_wave[2][16];
    __shared__ uint32_t s_carry[2];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    if (threadIdx.x < 2) s_carry[threadIdx.x] = 0;
    __syncthreads();
    for (int c = 0; c < nchunks; c += MESH_SCAN_TILE) {
        const int i0 = c + (int)threadIdx.x * MESH_SCAN_PER_LANE;
        uint32_t v[MESH_SCAN_PER_LANE], t[MESH_SCAN_PER_LANE], sv = 0, st = 0;
#pragma unroll
        for (int k = 0; k < MESH_SCAN_PER_LANE; k++) {
            v[k] = i0 + k < nchunks ? vbase[i0 + k] : 0u;
            t[k] = i0 + k < nchunks ? tbase[i0 + k] : 0u;
            sv += v[k];
            st += t[k];
        }
        uint32_t iv = sv, it = st; // inclusive over the lanes of the wave
        for (int o = 1; o < ADC_WAVE; o <<= 1) {
            const uint32_t uv = (uint32_t)__shfl_up((int)iv, o, ADC_WAVE), ut = (uint32_t)__shfl_up((int)it, o, ADC_WAVE);
            if (lane >= o) { iv += uv; it += ut; }
        }
        if (lane == ADC_WAVE - 1) { s_wave[0][wave] = iv; s_wave[1][wave] = it; }
        __syncthreads();
        uint32_t bv = s_carry[0], bt = s_carry[1], total_v = 0, total_t = 0;
        for (int w = 0; w < 16; w++) {
            const uint32_t wv = s_wave[0][w], wt = s_wave[1][w];
            if (w < wave) { bv += wv; bt += wt; }
            total_v += wv;
            total_t += wt;
        }
        bv += iv - sv; // entries of all lanes, waves and turns in front of this lane's first
        bt += it - st;
#pragma unroll
        for (int k = 0; k < MESH_SCAN_PER_LANE; k++)
            if (i0 + k < nchunks) {
                vbase[i0 + k] = bv;
                tbase[i0 + k] = bt;
                bv += v[k];
                bt += t[k];
            }
        __syncthreads();
        if (threadIdx.x == 0) { s_carry[0] += total_v; s_carry[1] += total_t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t nv = s_carry[0], nt = s_carry[1];
        rep[1] = nv;
        rep[2] = nt;
        if (counts) { counts[0] = nv; counts[1] = nt; }
    }
}

// the number of the vertex at lattice index Lc: the used points in front of it, from its own chunk's base and used word
__device__ __forceinline__ uint32_t mesh_vertex_number(const MeshArgs& g, int Lc)
{
    const int ch = Lc / ADC_WAVE, ln = Lc & (ADC_WAVE - 1);
    return g.vbase[ch] + (uint32_t)__popcll(g.used[ch] & ((1ull << ln) - 1ull));
}

__global__ __launch_bounds__(MESH_WG) void k_mesh_emit(const MeshArgs g)
{
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
#pragma unroll 1
    for (int k = 0; k < MESH_PER_WAVE; k++) {
        const int chunk = ((int)blockIdx.x * MESH_WAVES + wave) * MESH_PER_WAVE + k;
        if (chunk * ADC_WAVE >= g.Nl) continue; // (uniform in the wave)
        const int L = chunk * ADC_WAVE + lane;
        const bool in = L < g.Nl;
        const int j = L / g.Wl, i = L - j * g.Wl;
        if (g.vertices) {
            const unsigned long long um = g.used[chunk];
            const uint32_t at = g.vbase[chunk] + __builtin_amdgcn_mbcnt_hi((uint32_t)(um >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)um, 0u));
            if (((um >> lane) & 1ull) && at < g.vcap) { // (a used point lies inside the lattice)
                const int x = i * g.step, y = j * g.step;
                const size_t pixel = (size_t)y * (size_t)g.W + (size_t)x;
                float p[3];
                mesh_point(g.cam, x, y, __builtin_fabsf(g.disp[pixel]), p);
                uint4 pt;
                pt.x = __float_as_uint(p[0]);
                pt.y = __float_as_uint(p[1]);
                pt.z = __float_as_uint(p[2]);
                pt.w = mesh_colour(g.img, pixel);
                g.vertices[at] = pt;
                if (g.vindex) g.vindex[at] = (int32_t)pixel;
            }
        }
        if (g.triangles) {
            const uint32_t code = in ? (uint32_t)g.codes[L] : 0u;
            const unsigned long long t0 = __ballot((code & MESH_T0) != 0), t1 = __ballot((code & MESH_T1) != 0);
            const unsigned long long below = (1ull << lane) - 1ull;
            uint32_t rank = g.tbase[chunk] + (uint32_t)__popcll(t0 & below) + (uint32_t)__popcll(t1 & below);
            if (code && rank < g.tcap) {
                // an emitted triangle's corners lie inside the lattice: i + 1 < Wl, j + 1 < Hl
                uint32_t vn[4];
#pragma unroll
                for (int c = 0; c < 4; c++) vn[c] = mesh_code_uses(code, c) ? mesh_vertex_number(g, L + (c & 1) + (c >> 1) * g.Wl) : 0u;
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    if (!(code & (1u << t))) continue;
                    if (rank < g.tcap) {
                        int corner[3];
                        mesh_triangle_corners(code, t, corner);
                        uint32_t* out = g.triangles + (size_t)rank * 3;
                        out[0] = vn[corner[0]];
                        out[1] = vn[corner[1]];
                        out[2] = vn[corner[2]];
                    }
                    rank++;
                }
            }
        }
    }
}

static int mesh_chunks(int W, int H, int step)
{
    const long long Nl = (long long)mesh_lattice(W, step) * mesh_lattice(H, step);
    return (int)((Nl + ADC_WAVE - 1) / ADC_WAVE);
}

// one block for every step: the report words, two count arrays, the used words (8-byte aligned behind an even number of words), the codes
size_t adc_mesh_scratch_bytes(int W, int H)
{
    const size_t nch = (size_t)mesh_chunks(W, H, 1);
    return (MESH_REP_WORDS + 4 * nch) * sizeof(uint32_t) + (size_t)W * H;
}

static MeshArgs mesh_args(adc_handle* h, const AdcMeshReq& r)
{
    MeshArgs g;
    g.disp = r.disp;
    g.img = r.img;
    g.cam = mesh_cam(r.calib);
    g.max_diff = r.max_diff;
    g.step = r.step;
    g.W = h->p.W;
    g.Wl = mesh_lattice(h->p.W, r.step);
    g.Hl = mesh_lattice(h->p.H, r.step);
    g.Nl = g.Wl * g.Hl;
    const size_t nch = (size_t)mesh_chunks(h->p.W, h->p.H, r.step);
    g.rep = h->msh_words;
    g.vbase = h->msh_words + MESH_REP_WORDS;
    g.tbase = g.vbase + nch;
    g.used = reinterpret_cast<unsigned long long*>(g.tbase + nch);
    g.codes = r.triangles ? reinterpret_cast<uint8_t*>(g.used + nch) : nullptr;
    g.vertices = static_cast<uint4*>(r.vertices);
    g.vindex = r.vertex_index;
    g.triangles = r.triangles;
    g.vcap = r.vertex_capacity;
    g.tcap = r.triangle_capacity;
    g.counts = r.counts;
    return g;
}

hipError_t adc_launch_mesh_measure(adc_handle* h, const AdcMeshReq& r)
{
    if (r.step < 1 || r.step > ADC_MESH_MAX_STEP || !h->msh_words) return hipErrorInvalidValue;
    const MeshArgs g = mesh_args(h, r);
    hipLaunchKernelGGL(k_mesh_measure, dim3((unsigned)((g.Nl + MESH_TILE - 1) / MESH_TILE)), dim3(MESH_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_mesh_scan(adc_handle* h, const AdcMeshReq& r)
{
    const MeshArgs g = mesh_args(h, r);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, h->stream, g.vbase, g.tbase, mesh_chunks(h->p.W, h->p.H, r.step), g.rep, g.counts);
    return hipGetLastError();
}

hipError_t adc_launch_mesh_emit(adc_handle* h, const AdcMeshReq& r)
{
    const MeshArgs g = mesh_args(h, r);
    hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)((g.Nl + MESH_TILE - 1) / MESH_TILE)), dim3(MESH_WG), 0, h->stream, g);
    return hipGetLastError();
}
