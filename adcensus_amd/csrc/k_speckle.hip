// k_speckle.hip -- the optional speckle filter (include/adcensus_c_api.h: adc_set_speckle_filter, adc_filter_speckles_device):
// 4-connected component labelling of a float32 [H][W] map under the relation "both finite and fabsf(a - b) <= max_diff", then
// every component of at most max_size pixels becomes +inf.  DESIGN.md 4.8 has the formulation and the termination argument.
//
// Four launches whose grids depend on W and H only, no host read-back between them, and no workgroup ever waits for another one:
//   k_spk_runs     per 64-pixel piece of a row (one wave): parent[i] = first pixel of the pixel's run inside the piece (ballot
//                  over "not joined to the left neighbour"), -1 where the pixel is invalid; size[i] = 0; the stat words = 0
//   k_spk_merge    min-index union-find on the global parent array: a pixel joined to its upper neighbour unites with it unless
//                  the left neighbours already carry that link (pixel ~ left ~ upper-left ~ upper), and lane 0 unites its piece
//                  with the piece to the left.  atomicMin only: a parent never grows, so every find / union loop ends
//   k_spk_flatten  parent[i] = root (= the component's first pixel in raster order = the label); sizes by integer atomicAdd at
//                  the root, one per stretch of consecutive pixels (in raster order, 512 per wave) with the same root; components
//   k_spk_apply    size[root] <= max_size -> +inf (and ADC_PROV_SPECKLE in the provenance map), everything else keeps its bits;
//                  removed components / pixels.  Reads src, writes dst: in place for a caller's map, out of place behind a Match
// Roots are minima and sizes integer sums: nothing depends on the order of arrival.
#include "adc_internal.h"
#include "adc_device_fn.h"

#define SPK_WG 256
#define SPK_WAVES (SPK_WG / ADC_WAVE)
#define SPK_CHUNKS 8                                   // pieces of 64 consecutive pixels a wave of k_spk_flatten owns

__device__ __forceinline__ int spk_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool spk_joined(float a, float b, float max_diff)
{
    return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_fabsf(a - b) <= max_diff;
}

// parent[x] <= x always, and parent[x] == x only at a root: the walk strictly descends
__device__ __forceinline__ int spk_find(int32_t* parent, int x)
{
    int p = spk_load(parent + x);
    while (p != x) {
        x = p;
        p = spk_load(parent + x);
    }
    return x;
}

// Lock-free union towards the smaller root.  Every round that does not finish lowers a or b strictly (old < the root it
// replaced), so the loop ends; a link that loses the race is carried on with the value that won (the standard argument of
// the atomicMin union: the loser's partner is united with the winner's root in the next round).
__device__ __forceinline__ void spk_union(int32_t* parent, int a, int b)
{
    const int a0 = a, b0 = b;
    for (;;) {
        a = spk_find(parent, a);
        b = spk_find(parent, b);
        if (a == b) break;
        if (a < b) {
            const int old = atomicMin(parent + b, a);
            if (old == b) break;
            b = old;
        } else {
            const int old = atomicMin(parent + a, b);
            if (old == a) break;
            a = old;
        }
    }
    // shorten the two paths for whoever comes next (a root of the same component that is not above the pixel: safe)
    const int r = a < b ? a : b;
    if (spk_load(parent + a0) > r) atomicMin(parent + a0, r);
    if (spk_load(parent + b0) > r) atomicMin(parent + b0, r);
}

// wave c owns the pixels [x0, x0 + 64) of row y
__device__ __forceinline__ bool spk_piece(int W, int H, int* y, int* x0)
{
    const int cpr = (W + ADC_WAVE - 1) / ADC_WAVE;
    const long long c = (long long)blockIdx.x * SPK_WAVES + (int)threadIdx.x / ADC_WAVE;
    if (c >= (long long)cpr * H) return false;
    *y = (int)(c / cpr);
    *x0 = (int)(c - (long long)*y * cpr) * ADC_WAVE;
    return true;
}

__global__ __launch_bounds__(SPK_WG) void k_spk_runs(const float* __restrict__ src, int32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                      uint32_t* __restrict__ stats, int W, int H, float max_diff)
{
    if (blockIdx.x == 0 && threadIdx.x < 3) stats[threadIdx.x] = 0;
    int y, x0;
    if (!spk_piece(W, H, &y, &x0)) return;
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1);
    const int x = x0 + lane;
    const bool inb = x < W;
    const int i = y * W + x;
    const float d = inb ? src[i] : ADC_INVALID_FLOAT;
    const float dl = __shfl_up(d, 1, ADC_WAVE);
    const bool jl = lane > 0 && spk_joined(d, dl, max_diff);
    const unsigned long long heads = __ballot(!jl); // (lane 0 always)
    const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
    if (inb) {
        parent[i] = __builtin_isfinite(d) ? y * W + x0 + start : -1;
        size[i] = 0;
    }
}

__global__ __launch_bounds__(SPK_WG) void k_spk_merge(const float* __restrict__ src, int32_t* parent, int W, int H, float max_diff)
{
    int y, x0;
    if (!spk_piece(W, H, &y, &x0)) return;
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1);
    const int x = x0 + lane;
    const bool inb = x < W;
    const int i = y * W + x;
    const float INF = ADC_INVALID_FLOAT;
    const float d = inb ? src[i] : INF;
    const float u = (inb && y > 0) ? src[i - W] : INF;
    float dl = __shfl_up(d, 1, ADC_WAVE), ul = __shfl_up(u, 1, ADC_WAVE);
    if (lane == 0) {
        dl = x > 0 ? src[i - 1] : INF;
        ul = (x > 0 && y > 0) ? src[i - W - 1] : INF;
    }
    const bool ju = spk_joined(d, u, max_diff), jl = spk_joined(d, dl, max_diff);
    // pixel ~ left ~ upper-left ~ upper: the left pixel's own link (or, by induction along the row, its left neighbours')
    // already joins the two rows here
    const bool carried = jl && spk_joined(dl, ul, max_diff) && spk_joined(ul, u, max_diff);
    if (ju && !carried) spk_union(parent, i, i - W);
    if (lane == 0 && jl) spk_union(parent, i, i - 1);
}

__global__ __launch_bounds__(SPK_WG) void k_spk_flatten(int32_t* parent, uint32_t* __restrict__ size, uint32_t* __restrict__ stats,
                                                         int32_t* __restrict__ labels, int P)
{
    __shared__ uint32_t s_roots[SPK_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const long long base = ((long long)blockIdx.x * SPK_WAVES + wave) * (ADC_WAVE * SPK_CHUNKS);
    int carry_root = -1;      // the stretch of equal roots that is still open at the end of the last piece (wave-uniform)
    uint32_t carry_cnt = 0, roots = 0;
    for (int k = 0; k < SPK_CHUNKS; k++) {
        const long long i = base + k * ADC_WAVE + lane;
        int r = -1;
        if (i < P) {
            const int p = spk_load(parent + i);
            if (p >= 0) {
                r = spk_find(parent, p);
                // (a concurrent find that passes through here reads the old parent or the root: both lie on its way up)
                if (r != p) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (labels) labels[i] = r;
        }
        roots += (uint32_t)__popcll(__ballot(r >= 0 && r == (int)i));
        int prev = __shfl_up(r, 1, ADC_WAVE);
        if (lane == 0) prev = carry_root;
        const unsigned long long heads = __ballot(r != prev);
        if (heads == 0) { // the whole piece continues the open stretch
            carry_cnt += ADC_WAVE;
            continue;
        }
        const int first = __builtin_ctzll(heads), last = 63 - __builtin_clzll(heads);
        if (lane == 0 && carry_root >= 0) atomicAdd(size + carry_root, carry_cnt + (uint32_t)first);
        if (((heads >> lane) & 1ull) && lane != last && r >= 0) {
            const unsigned long long above = heads & ~(~0ull >> (63 - lane)); // heads behind this lane (lane < 63 here: it is not the last head)
            atomicAdd(size + r, (uint32_t)(__builtin_ctzll(above) - lane));
        }
        carry_root = __shfl(r, last, ADC_WAVE);
        carry_cnt = (uint32_t)(ADC_WAVE - last);
    }
    if (lane == 0 && carry_root >= 0) atomicAdd(size + carry_root, carry_cnt);
    if (lane == 0) s_roots[wave] = roots;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < SPK_WAVES; w++) t += s_roots[w];
        if (t) atomicAdd(stats + 0, t);
    }
}

__global__ __launch_bounds__(SPK_WG) void k_spk_apply(const float* src, float* dst, const int32_t* __restrict__ parent,
                                                       const uint32_t* __restrict__ size, uint32_t* __restrict__ stats, uint8_t* __restrict__ prov,
                                                       int P, int max_size)
{
    __shared__ uint32_t s_px[SPK_WAVES], s_comp[SPK_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const long long i = (long long)blockIdx.x * SPK_WG + threadIdx.x;
    bool rm = false, root = false;
    if (i < P) {
        const int r = parent[i];
        rm = r >= 0 && size[r] <= (uint32_t)max_size;
        root = rm && r == (int)i;
        if (rm) dst[i] = ADC_INVALID_FLOAT;
        else if (dst != src) dst[i] = src[i];
        if (prov) {
            const uint8_t v = prov[i], nv = rm ? (uint8_t)(v | ADC_PROV_SPECKLE) : (uint8_t)(v & ~ADC_PROV_SPECKLE);
            if (nv != v) prov[i] = nv;
        }
    }
    const uint32_t px = (uint32_t)__popcll(__ballot(rm)), comp = (uint32_t)__popcll(__ballot(root));
    if (lane == 0) { s_px[wave] = px; s_comp[wave] = comp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (int w = 0; w < SPK_WAVES; w++) { a += s_comp[w]; b += s_px[w]; }
        if (a) atomicAdd(stats + 1, a);
        if (b) atomicAdd(stats + 2, b);
    }
}

// ints of the scratch: parent [P], size [P], then the three stat words (components, removed components, removed pixels)
size_t adc_speckle_scratch_words(int W, int H) { return 2 * (size_t)W * H + 4; }

// The launchers: src / dst are device-resident maps of the handle's geometry (dst == src: in place).  capi.hip orders them and
// owns every other HIP call of the path.
static unsigned spk_piece_grid(const adc_handle* h)
{
    const long long pieces = (long long)((h->p.W + ADC_WAVE - 1) / ADC_WAVE) * h->p.H;
    return (unsigned)((pieces + SPK_WAVES - 1) / SPK_WAVES);
}

hipError_t adc_launch_speckle_runs(adc_handle* h, const float* src, float max_diff)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    uint32_t* size = reinterpret_cast<uint32_t*>(h->sp_parent + P);
    hipLaunchKernelGGL(k_spk_runs, dim3(spk_piece_grid(h)), dim3(SPK_WG), 0, h->stream, src, h->sp_parent, size, size + P, h->p.W, h->p.H, max_diff);
    return hipGetLastError();
}

hipError_t adc_launch_speckle_merge(adc_handle* h, const float* src, float max_diff)
{
    hipLaunchKernelGGL(k_spk_merge, dim3(spk_piece_grid(h)), dim3(SPK_WG), 0, h->stream, src, h->sp_parent, h->p.W, h->p.H, max_diff);
    return hipGetLastError();
}

hipError_t adc_launch_speckle_flatten(adc_handle* h, int32_t* labels)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    uint32_t* size = reinterpret_cast<uint32_t*>(h->sp_parent + P);
    const size_t per_wg = (size_t)SPK_WG * SPK_CHUNKS;
    hipLaunchKernelGGL(k_spk_flatten, dim3((unsigned)((P + per_wg - 1) / per_wg)), dim3(SPK_WG), 0, h->stream, h->sp_parent, size, size + P, labels, (int)P);
    return hipGetLastError();
}

hipError_t adc_launch_speckle_apply(adc_handle* h, const float* src, float* dst, uint8_t* prov, int max_size)
{
    const size_t P = (size_t)h->p.W * h->p.H;
    uint32_t* size = reinterpret_cast<uint32_t*>(h->sp_parent + P);
    hipLaunchKernelGGL(k_spk_apply, dim3((unsigned)((P + SPK_WG - 1) / SPK_WG)), dim3(SPK_WG), 0, h->stream, src, dst, h->sp_parent, size, size + P, prov,
                       (int)P, max_size);
    return hipGetLastError();
}
