// k_voxel.hip -- the voxel-grid filter of the cloud (include/adcensus_c_api.h: adc_set_cloud_voxel_grid; voxel_point.h holds the
// per-point arithmetic, tests/voxel_ref.py the definition in numpy).  With a grid set these launches replace the cloud part of
// k_out_measure / k_out_scan / k_out_emit; depth and the 8-bit image keep their kernels.
//
// An open-addressing hash table of 64-byte slots, capacity the smallest power of two >= 2 * W * H (load factor <= 0.5), cleared to
// zero by one hipMemsetAsync in front of the launches:
//   VoxSlot   key + 1 (0 = empty: keys have 63 bits) | ~leader (0 = none: atomicMax of the complement is the minimum) | n | Sq[3] | Srgb[3]
// Four launches on the object stream, none of which waits for another lane, wave or workgroup of its own launch:
//   k_vox_insert  a pixel's point, crop, key; runs of equal keys among the 64 consecutive pixels of a wave's chunk are summed in the
//                 wave (segmented shuffle sums: every sum is an integer, so any grouping is exact), the first lane of a run finds or
//                 claims the key's slot (64-bit compare-and-swap, linear probing, at most `capacity` steps: the table can never fill)
//                 and issues ONE set of atomics for the run; every kept pixel records its slot (4 bytes); valid / kept counts per tile
//   k_vox_count   a pixel is its voxel's leader iff the slot's leader word is its raster index: leaders per tile, and the slot
//                 word of every other pixel becomes VOX_NO_SLOT (the emit then gathers for leaders only)
//   k_vox_scan    one workgroup, k_out_scan's form: exclusive scan of the leader counts; totals of the three report words
//   k_vox_emit    a leader's position is the raster rank of its flag (k_out_emit's form): it reads its slot's aggregate and writes
//                 one 16-byte record below the capacity
// Leaders are raster indices, so the records come out in ascending order of leader.
#include "adc_internal.h"
#include "adc_device_fn.h"
#include "voxel_point.h"

#define VOX_WG 256
#define VOX_WAVES (VOX_WG / ADC_WAVE)
#define VOX_PER_WAVE 4
#define VOX_TILE (VOX_WG * VOX_PER_WAVE) // pixels per workgroup: wave w owns [w * 256, w * 256 + 256) of the tile
#define VOX_NO_SLOT 0xffffffffu

struct VoxSlot {
    unsigned long long key1;   // key + 1
    uint32_t nleader;          // ~(lowest raster index)
    uint32_t n;
    unsigned long long sq[3];
    unsigned long long sc[3];  // r, g, b
};
static_assert(sizeof(VoxSlot) == 64, "one slot is 64 bytes");

struct VoxArgs {
    const float* disp;
    const uint8_t* img;    // left image, B,G,R per pixel
    VoxSlot* table;
    uint32_t mask;         // slots - 1
    uint32_t* slot_of;     // [P]
    uint32_t* words;       // [0] voxels, [1] points_valid, [2] points_kept, [4 ...] leaders per tile -> bases, then valid and kept per tile
    uint4* cloud;
    uint32_t* count_out;   // the caller's device word, may be null
    uint32_t capacity;
    int P, W, ntiles;
    float fb, focal, cx, cy, doffs;
    VoxGrid grid;
};

__device__ __forceinline__ uint32_t vox_hash(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k;
}

// the slot of a key: found, or claimed from empty; VOX_NO_SLOT only if every slot holds another key (cannot happen at load <= 0.5)
__device__ __forceinline__ uint32_t vox_find_slot(const VoxArgs& g, unsigned long long key)
{
    const unsigned long long want = key + 1ull;
    uint32_t s = vox_hash(key) & g.mask;
    for (uint32_t step = 0; step <= g.mask; step++) {
        unsigned long long* p = &g.table[s].key1;
        unsigned long long cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) cur = atomicCAS(p, 0ull, want); // (the value found: 0 = this lane has claimed the slot)
        if (cur == 0ull || cur == want) return s;
        s = (s + 1u) & g.mask;
    }
    return VOX_NO_SLOT;
}

__global__ __launch_bounds__(VOX_WG) void k_vox_insert(const VoxArgs g)
{
    __shared__ uint32_t s_valid[VOX_WAVES], s_kept[VOX_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int base = (int)blockIdx.x * VOX_TILE + wave * (ADC_WAVE * VOX_PER_WAVE);
    uint32_t nvalid = 0, nkept = 0;
    for (int k = 0; k < VOX_PER_WAVE; k++) {
        const int i = base + k * ADC_WAVE + lane;
        bool valid = false, kept = false;
        unsigned long long key = VOX_KEY_NONE;
        uint32_t v[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u}; // n, q x y z, r g b
        if (i < g.P) {
            const float a = __builtin_fabsf(g.disp[i]);
            const float s = a + g.doffs;
            valid = __builtin_isfinite(a) && s > 0.0f;
            if (valid) {
                const int y = i / g.W, x = i - y * g.W;
                const float Z = g.fb / s;
                const float X = (((float)x - g.cx) * Z) / g.focal;
                const float Y = (((float)y - g.cy) * Z) / g.focal;
                kept = vox_point(g.grid, X, Y, Z, &key, &v[1]);
                if (kept) {
                    const uint8_t* c = g.img + (size_t)i * 3;
                    v[0] = 1u; v[4] = c[2]; v[5] = c[1]; v[6] = c[0];
                } else {
                    key = VOX_KEY_NONE;
                }
            }
        }
        nvalid += (uint32_t)__popcll(__ballot(valid));
        const unsigned long long keptmask = __ballot(kept);
        nkept += (uint32_t)__popcll(keptmask);
        if (keptmask == 0ull) { // (wave-uniform) nothing to insert; the tail of the map writes nothing
            if (i < g.P) g.slot_of[i] = VOX_NO_SLOT;
            continue;
        }
        // runs of equal keys: a lane is the head of its run iff it is lane 0, not kept, or its key differs from its left neighbour's
        const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
        const uint32_t plo = (uint32_t)__shfl_up((int)klo, 1, ADC_WAVE), phi = (uint32_t)__shfl_up((int)khi, 1, ADC_WAVE);
        const bool head = lane == 0 || !kept || plo != klo || phi != khi;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == ADC_WAVE - 1 ? 0ull : heads >> (lane + 1);
        const int end = above ? lane + __builtin_ctzll(above) : ADC_WAVE - 1; // last lane of this lane's run
        const int first = 63 - __builtin_clzll(heads & ((2ull << lane) - 1ull)); // its head (bit 0 is always set)
        // segmented suffix sums: after the step with offset o a lane holds the sum over [lane, min(lane + 2o - 1, end)]
        for (int o = 1; o < ADC_WAVE; o <<= 1) {
            const bool take = lane + o <= end;
#pragma unroll
            for (int c = 0; c < 7; c++) {
                const uint32_t t = (uint32_t)__shfl_down((int)v[c], o, ADC_WAVE);
                if (take) v[c] += t;
            }
        }
        uint32_t slot = VOX_NO_SLOT;
        if (head && kept) {
            slot = vox_find_slot(g, key);
            if (slot != VOX_NO_SLOT) {
                VoxSlot* p = &g.table[slot];
                atomicMax(&p->nleader, ~(uint32_t)i); // (the head is the run's lowest raster index)
                atomicAdd(&p->n, v[0]);
                atomicAdd(&p->sq[0], (unsigned long long)v[1]);
                atomicAdd(&p->sq[1], (unsigned long long)v[2]);
                atomicAdd(&p->sq[2], (unsigned long long)v[3]);
                atomicAdd(&p->sc[0], (unsigned long long)v[4]);
                atomicAdd(&p->sc[1], (unsigned long long)v[5]);
                atomicAdd(&p->sc[2], (unsigned long long)v[6]);
            }
        }
        slot = (uint32_t)__shfl((int)slot, first, ADC_WAVE);
        if (i < g.P) g.slot_of[i] = kept ? slot : VOX_NO_SLOT;
    }
    if (lane == 0) { s_valid[wave] = nvalid; s_kept[wave] = nkept; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t tv = 0, tk = 0;
    for (int w = 0; w < VOX_WAVES; w++) { tv += s_valid[w]; tk += s_kept[w]; }
    g.words[4 + g.ntiles + blockIdx.x] = tv;
    g.words[4 + 2 * g.ntiles + blockIdx.x] = tk;
}

__global__ __launch_bounds__(VOX_WG) void k_vox_count(const VoxArgs g)
{
    __shared__ uint32_t s_cnt[VOX_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int base = (int)blockIdx.x * VOX_TILE + wave * (ADC_WAVE * VOX_PER_WAVE);
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < VOX_PER_WAVE; k++) {
        const int i = base + k * ADC_WAVE + lane;
        bool leader = false;
        if (i < g.P) {
            const uint32_t slot = g.slot_of[i];
            if (slot != VOX_NO_SLOT) {
                leader = g.table[slot].nleader == ~(uint32_t)i;
                if (!leader) g.slot_of[i] = VOX_NO_SLOT;
            }
        }
        cnt += (uint32_t)__popcll(__ballot(leader));
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t t = 0;
    for (int w = 0; w < VOX_WAVES; w++) t += s_cnt[w];
    g.words[4 + blockIdx.x] = t;
}

__device__ __forceinline__ uint32_t vox_wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, ADC_WAVE);
    return v;
}

// One workgroup of 1024: leader counts -> exclusive prefix sums in place, chunk by chunk with a carry (k_out_scan's form); the
// total goes to words[0] and the caller's device word, the sums of the valid / kept tile counts to words[1] and [2].
__global__ __launch_bounds__(1024) void k_vox_scan(uint32_t* __restrict__ words, int ntiles, uint32_t* __restrict__ count_out)
{
    __shared__ uint32_t s_wave[16], s_v[16], s_k[16];
    __shared__ uint32_t s_carry;
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    uint32_t* tiles = words + 4;
    const uint32_t* tvalid = tiles + ntiles;
    const uint32_t* tkept = tiles + 2 * ntiles;
    uint32_t nv = 0, nk = 0;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int c = 0; c < ntiles; c += 1024) {
        const int i = c + (int)threadIdx.x;
        const uint32_t v = i < ntiles ? tiles[i] : 0u;
        if (i < ntiles) { nv += tvalid[i]; nk += tkept[i]; }
        uint32_t incl = v;
        for (int o = 1; o < ADC_WAVE; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o, ADC_WAVE);
            if (lane >= o) incl += t;
        }
        if (lane == ADC_WAVE - 1) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry, total = 0;
        for (int w = 0; w < 16; w++) {
            const uint32_t t = s_wave[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < ntiles) tiles[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += total;
        __syncthreads();
    }
    nv = vox_wave_sum(nv);
    nk = vox_wave_sum(nk);
    if (lane == 0) { s_v[wave] = nv; s_k[wave] = nk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tv = 0, tk = 0;
        for (int w = 0; w < 16; w++) { tv += s_v[w]; tk += s_k[w]; }
        words[0] = s_carry;
        words[1] = tv;
        words[2] = tk;
        if (count_out) *count_out = s_carry;
    }
}

__global__ __launch_bounds__(VOX_WG) void k_vox_emit(const VoxArgs g)
{
    __shared__ uint32_t s_cnt[VOX_WAVES];
    const int lane = (int)threadIdx.x & (ADC_WAVE - 1), wave = (int)threadIdx.x / ADC_WAVE;
    const int base = (int)blockIdx.x * VOX_TILE + wave * (ADC_WAVE * VOX_PER_WAVE);
    uint32_t slot[VOX_PER_WAVE];
    unsigned long long mask[VOX_PER_WAVE];
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < VOX_PER_WAVE; k++) {
        const int i = base + k * ADC_WAVE + lane;
        slot[k] = i < g.P ? g.slot_of[i] : VOX_NO_SLOT; // (k_vox_count left a slot at the leaders only)
        mask[k] = __ballot(slot[k] != VOX_NO_SLOT);
        cnt += (uint32_t)__popcll(mask[k]);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    uint32_t pos = g.words[4 + blockIdx.x]; // the tile's base: leaders of all tiles before it
    for (int w = 0; w < wave; w++) pos += s_cnt[w];
#pragma unroll
    for (int k = 0; k < VOX_PER_WAVE; k++) {
        const unsigned long long m = mask[k];
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const uint32_t at = pos + below;
        if (slot[k] != VOX_NO_SLOT && at < g.capacity) {
            const VoxSlot* p = &g.table[slot[k]];
            const unsigned long long sq[3] = {p->sq[0], p->sq[1], p->sq[2]};
            const unsigned long long sc[3] = {p->sc[0], p->sc[1], p->sc[2]};
            uint32_t w[4];
            vox_record(p->key1 - 1ull, p->n, sq, sc, g.grid.leaf, w);
            uint4 pt;
            pt.x = w[0]; pt.y = w[1]; pt.z = w[2]; pt.w = w[3];
            g.cloud[at] = pt;
        }
        pos += (uint32_t)__popcll(m);
    }
}

// slots of the table: the smallest power of two >= 2 * W * H
size_t adc_voxel_table_slots(int W, int H)
{
    const size_t need = 2 * (size_t)W * H;
    size_t n = 2;
    while (n < need) n <<= 1;
    return n;
}
size_t adc_voxel_table_bytes(int W, int H) { return adc_voxel_table_slots(W, H) * sizeof(VoxSlot); }
static int vox_tiles(int P) { return (P + VOX_TILE - 1) / VOX_TILE; }
size_t adc_voxel_words_bytes(int W, int H) { return (4 + 3 * (size_t)vox_tiles(W * H)) * sizeof(uint32_t); }

static VoxArgs vox_args(adc_handle* h, const float* disp, const uint8_t* img)
{
    const AdcOutReq& r = h->fly.req.out;
    VoxArgs g;
    g.disp = disp;
    g.img = img;
    g.table = static_cast<VoxSlot*>(h->vox_table);
    g.mask = (uint32_t)(adc_voxel_table_slots(h->p.W, h->p.H) - 1);
    g.slot_of = h->vox_slot;
    g.words = h->vox_words;
    g.cloud = static_cast<uint4*>(r.cloud);
    g.count_out = r.cloud_count;
    g.capacity = r.capacity;
    g.P = h->p.W * h->p.H;
    g.W = h->p.W;
    g.ntiles = vox_tiles(g.P);
    g.fb = r.fb; g.focal = r.calib.focal_px; g.cx = r.calib.cx; g.cy = r.calib.cy; g.doffs = r.calib.doffs;
    g.grid = h->vox_grid;
    return g;
}

hipError_t adc_launch_vox_insert(adc_handle* h, const float* disp, const uint8_t* img)
{
    const VoxArgs g = vox_args(h, disp, img);
    hipLaunchKernelGGL(k_vox_insert, dim3((unsigned)g.ntiles), dim3(VOX_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_vox_count(adc_handle* h)
{
    const VoxArgs g = vox_args(h, nullptr, nullptr);
    hipLaunchKernelGGL(k_vox_count, dim3((unsigned)g.ntiles), dim3(VOX_WG), 0, h->stream, g);
    return hipGetLastError();
}

hipError_t adc_launch_vox_scan(adc_handle* h)
{
    hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(1024), 0, h->stream, h->vox_words, vox_tiles(h->p.W * h->p.H), h->fly.req.out.cloud_count);
    return hipGetLastError();
}

hipError_t adc_launch_vox_emit(adc_handle* h)
{
    const VoxArgs g = vox_args(h, nullptr, nullptr);
    hipLaunchKernelGGL(k_vox_emit, dim3((unsigned)g.ntiles), dim3(VOX_WG), 0, h->stream, g);
    return hipGetLastError();
}
