// emul_mem.cpp -- adcensus_amd/csrc/dev_mem.h (the owner of a handle's device and pinned memory) on the CPU: malloc / free in place of
// the HIP calls, a switch that fails the n-th allocation, a live count of its own.  Every block carries its kind in a header, so a
// block freed by the other kind's function is seen.  Built with -fsanitize=address,undefined: a leak, a double free or an overrun of
// the registry ends the program.
//   emul_mem <case>   prints one line of key=value facts; the last one is violations=<n> (tests/test_emul_mem.py asserts on them)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../adcensus_amd/csrc/dev_mem.h"

static long g_calls, g_fail_at, g_live, g_allocs[2], g_frees[2], g_wrong_frees, g_last_bytes;
static int g_violations;
#define CHECK(cond) do { if (!(cond)) { g_violations++; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)
static const int EMU_ERROR = 7; // handed back by dev_mem.h unchanged

struct Emu {
    static int alloc(void** p, size_t bytes, int kind)
    {
        if (++g_calls == g_fail_at) return EMU_ERROR; // (like an injected HIP failure: *p is not written)
        unsigned char* b = static_cast<unsigned char*>(malloc(bytes + 16));
        if (!b) abort();
        b[0] = (unsigned char)(0xD0 + kind);
        *p = b + 16;
        g_live++; g_allocs[kind]++; g_last_bytes = (long)bytes;
        return 0;
    }
    static void release(void* p, int kind)
    {
        unsigned char* b = static_cast<unsigned char*>(p) - 16;
        if (b[0] != 0xD0 + kind) g_wrong_frees++;
        g_live--; g_frees[kind]++;
        free(b);
    }
    static int alloc_device(void** p, size_t bytes) { return alloc(p, bytes, 0); }
    static int alloc_pinned(void** p, size_t bytes) { return alloc(p, bytes, 1); }
    static void free_device(void* p) { release(p, 0); }
    static void free_pinned(void* p) { release(p, 1); }
};

// a handle in small: typed pointer fields and capacities around the registry, cleared with memset like adc_create does
struct Fake {
    DevMemOwner mem;
    uint8_t *a, *b;
    float* c;
    uint64_t* d;
    void* e;
    int32_t* f;
    size_t c_cap, d_cap, f_cap;
    uint32_t* many[DEV_MEM_SLOTS + 4];
};
static Fake* fake_new() { Fake* h = static_cast<Fake*>(malloc(sizeof(Fake))); if (!h) abort(); memset(h, 0, sizeof(*h)); return h; }
static void reset_counts() { g_calls = g_fail_at = g_allocs[0] = g_allocs[1] = g_frees[0] = g_frees[1] = g_wrong_frees = 0; }

static void case_once(void)
{
    Fake* h = fake_new();
    uint8_t preset[4];
    h->a = preset; // a field that is set: no call, and nothing registered that release_all would free
    CHECK(dev_mem_once<Emu>(&h->mem, &h->a, 100) == 0 && g_calls == 0 && h->a == preset && h->mem.count == 0);
    CHECK(dev_mem_once<Emu>(&h->mem, &h->b, 100) == 0 && g_calls == 1 && h->b && g_last_bytes == 100);
    uint8_t* first = h->b;
    CHECK(dev_mem_once<Emu>(&h->mem, &h->b, 999) == 0 && g_calls == 1 && h->b == first);
    CHECK(dev_mem_once_pinned<Emu>(&h->mem, &h->e, 64) == 0 && g_calls == 2 && g_allocs[1] == 1);
    printf("calls=%ld registered=%d ", g_calls, h->mem.count);
    dev_mem_release_all<Emu>(&h->mem);
    CHECK(h->a == preset && !h->b && !h->e);
    free(h);
}

static void case_fail_retry(void)
{
    Fake* h = fake_new();
    g_fail_at = 1;
    CHECK(dev_mem_once<Emu>(&h->mem, &h->a, 10) == EMU_ERROR && !h->a && g_live == 0);
    CHECK(dev_mem_once<Emu>(&h->mem, &h->a, 10) == 0 && h->a && g_live == 1 && h->mem.count == 1); // (registered once, not twice)
    g_fail_at = 3;
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 8, 4) == EMU_ERROR && !h->c && h->c_cap == 0);
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 8, 4) == 0 && h->c && h->c_cap == 8 && g_last_bytes == 32);
    g_fail_at = 5; // a REGROW that fails: the old block is gone, field and capacity say so
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 9, 4) == EMU_ERROR && !h->c && h->c_cap == 0 && g_live == 1);
    CHECK(dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 2, 8) == 0 && h->d_cap == 2);
    g_fail_at = 7;
    CHECK(dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 3, 8) == EMU_ERROR && !h->d && h->d_cap == 0);
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 2, 4) == 0 && h->c_cap == 2);
    printf("calls=%ld live_before_release=%ld registered=%d ", g_calls, g_live, h->mem.count);
    dev_mem_release_all<Emu>(&h->mem);
    free(h);
}

static void case_grow_sequence(void)
{
    Fake* h = fake_new();
    const size_t seq[4] = {8, 4, 8, 16};
    long sizes[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        const long before = g_calls;
        CHECK(dev_mem_grow<Emu>(&h->mem, &h->d, &h->d_cap, seq[i], sizeof(uint64_t)) == 0);
        sizes[i] = g_calls > before ? g_last_bytes : 0;
        if (h->d) h->d[h->d_cap - 1] = 1; // (the block holds what the capacity says: the sanitizer checks)
    }
    printf("allocs=%ld frees=%ld bytes=%ld,%ld,%ld,%ld cap=%zu ", g_allocs[0], g_frees[0], sizes[0], sizes[1], sizes[2], sizes[3], h->d_cap);
    dev_mem_release_all<Emu>(&h->mem);
    free(h);
}

static void case_kinds(void)
{
    Fake* h = fake_new();
    CHECK(dev_mem_once<Emu>(&h->mem, &h->a, 1) == 0);
    CHECK(dev_mem_once_pinned<Emu>(&h->mem, &h->b, 2) == 0);
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 3, 4) == 0);
    CHECK(dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 4, 8) == 0);
    CHECK(dev_mem_once<Emu>(&h->mem, &h->e, 5) == 0);
    CHECK(dev_mem_once_pinned<Emu>(&h->mem, &h->f, 6) == 0);
    CHECK(dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 40, 8) == 0); // a regrow frees by the kind it was allocated with
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 30, 4) == 0);
    dev_mem_release<Emu>(&h->mem, &h->b);                                   // ... and so does giving one buffer back early
    CHECK(!h->b && g_frees[1] == 2 && h->mem.count == 6);
    dev_mem_release<Emu>(&h->mem, &h->b);                                   // (nothing left to give back)
    CHECK(g_frees[1] == 2);
    dev_mem_release_all<Emu>(&h->mem);
    printf("device_allocs=%ld pinned_allocs=%ld device_frees=%ld pinned_frees=%ld wrong_frees=%ld ", g_allocs[0], g_allocs[1], g_frees[0], g_frees[1], g_wrong_frees);
    free(h);
}

static void case_release_all(void)
{
    Fake* h = fake_new();
    g_fail_at = 2;
    CHECK(dev_mem_once<Emu>(&h->mem, &h->a, 10) == 0);
    CHECK(dev_mem_once_pinned<Emu>(&h->mem, &h->b, 10) == EMU_ERROR);        // failed and never retried: registered, null
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 4, 4) == 0);
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 40, 4) == 0);         // regrown
    CHECK(dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 4, 8) == 0);
    g_fail_at = g_calls + 1;
    CHECK(dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 5, 8) != 0);   // regrow failed: null with capacity 0
    CHECK(dev_mem_once<Emu>(&h->mem, &h->e, 1) == 0);
    const long live = g_live;
    dev_mem_release_all<Emu>(&h->mem);
    const long frees = g_frees[0] + g_frees[1], calls = g_calls;
    CHECK(!h->a && !h->b && !h->c && !h->d && !h->e && !h->f);
    dev_mem_release_all<Emu>(&h->mem); // again: nothing to do
    printf("live_before=%ld live_after=%ld second_release_frees=%ld second_release_calls=%ld wrong_frees=%ld ", live, g_live, g_frees[0] + g_frees[1] - frees,
           g_calls - calls, g_wrong_frees);
    free(h);
}

static void case_full(void)
{
    Fake* h = fake_new();
    int ok = 0, full = 0;
    for (int i = 0; i < DEV_MEM_SLOTS + 4; i++) {
        const long before = g_calls;
        const int rc = dev_mem_once<Emu>(&h->mem, &h->many[i], 4, (i & 1) ? DEV_MEM_PINNED : DEV_MEM_DEVICE);
        if (rc == 0) ok++;
        else { full += rc == DEV_MEM_FULL; CHECK(g_calls == before && !h->many[i]); } // refused: no allocation, nothing to lose
    }
    size_t cap = 0;
    CHECK(dev_mem_grow<Emu>(&h->mem, &h->c, &cap, 3, 4) == DEV_MEM_FULL && !h->c && cap == 0);
    CHECK(dev_mem_once<Emu>(&h->mem, &h->many[0], 4) == 0);                              // a registered field is still served
    dev_mem_release<Emu>(&h->mem, &h->many[1]);
    CHECK(dev_mem_once_pinned<Emu>(&h->mem, &h->many[1], 4) == 0 && h->many[1]);         // ... also when it has to be allocated again
    printf("slots=%d accepted=%d refused_full=%d registered=%d live_before_release=%ld ", DEV_MEM_SLOTS, ok, full, h->mem.count, g_live);
    dev_mem_release_all<Emu>(&h->mem);
    CHECK(g_wrong_frees == 0);
    free(h);
}

// twelve slots the way a handle uses them: fixed buffers, growing ones, both kinds; a call that fails is followed by the others
static int script(Fake* h)
{
    int failed = 0;
    failed += dev_mem_once<Emu>(&h->mem, &h->a, 100) != 0;
    failed += dev_mem_once<Emu>(&h->mem, &h->b, 50) != 0;
    failed += dev_mem_once_pinned<Emu>(&h->mem, &h->e, 64) != 0;
    failed += dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 8, 4) != 0;
    failed += dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 4, 4) != 0;
    failed += dev_mem_grow<Emu>(&h->mem, &h->c, &h->c_cap, 16, 4) != 0;
    failed += dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 3, 8) != 0;
    failed += dev_mem_grow_pinned<Emu>(&h->mem, &h->d, &h->d_cap, 9, 8) != 0;
    for (int i = 0; i < 6; i++) failed += dev_mem_once<Emu>(&h->mem, &h->many[i], 8 + i, (i & 1) ? DEV_MEM_PINNED : DEV_MEM_DEVICE) != 0;
    failed += dev_mem_grow<Emu>(&h->mem, &h->f, &h->f_cap, 5, 4) != 0;
    return failed;
}
static void case_sweep(void)
{
    Fake* h = fake_new();
    CHECK(script(h) == 0);
    const long N = g_calls;
    CHECK(h->mem.count == 12);
    dev_mem_release_all<Emu>(&h->mem);
    free(h);
    CHECK(g_live == 0);
    int runs = 0, leaks = 0;
    for (long n = 1; n <= N; n++)
        for (int retry = 0; retry < 2; retry++) { // released right behind the failure, or after a second, clean pass over the script
            h = fake_new();
            reset_counts();
            g_fail_at = n;
            CHECK(script(h) >= 1);
            if (retry) { CHECK(script(h) == 0); CHECK(h->a && h->b && h->c && h->d && h->e && h->f && h->c_cap == 16 && h->d_cap == 9 && h->f_cap == 5); }
            dev_mem_release_all<Emu>(&h->mem);
            leaks += g_live != 0;
            CHECK(g_wrong_frees == 0 && g_allocs[0] == g_frees[0] && g_allocs[1] == g_frees[1]);
            free(h);
            runs++;
        }
    printf("script_allocations=%ld runs=%d runs_with_live_buffers=%d ", N, runs, leaks);
}

int main(int argc, char** argv)
{
    static const struct { const char* name; void (*run)(void); } cases[] = {{"once", case_once}, {"fail_retry", case_fail_retry},
        {"grow_sequence", case_grow_sequence}, {"kinds", case_kinds}, {"release_all", case_release_all}, {"full", case_full}, {"sweep", case_sweep}};
    for (const auto& c : cases)
        if (argc == 2 && !strcmp(argv[1], c.name)) {
            c.run();
            printf("live=%ld violations=%d\n", g_live, g_violations);
            return g_violations ? 1 : 0;
        }
    fprintf(stderr, "usage: emul_mem once|fail_retry|grow_sequence|kinds|release_all|full|sweep\n");
    return 2;
}
