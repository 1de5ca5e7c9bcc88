// dev_mem.h -- who owns a handle's device and pinned memory.  Host-only C++ shared by the product and the CPU tests
// (tests/emul/emul_mem.cpp): no HIP header, no handle.  The functions are templates over a type M the includer supplies:
//     static int  M::alloc_device(void** p, size_t bytes);   static void M::free_device(void* p);
//     static int  M::alloc_pinned(void** p, size_t bytes);   static void M::free_pinned(void* p);
// (alloc: 0 = done, anything else = the includer's own error code, handed back unchanged; capi.hip: the HIP calls).
//
// A buffer is a pointer FIELD of the handle.  The first allocation of a field registers the field's ADDRESS with its kind; the
// handle lives on the heap and never moves, so the registry stays right however often a field is regrown, and the typed fields keep
// their names.  All bytes zero = an empty registry (adc_create clears the handle with memset).  dev_mem_release_all frees what the
// registered fields point to: a field that is allocated in any other way is not freed by anybody.
#pragma once
#include <stddef.h>

#define DEV_MEM_SLOTS 192 // a handle registers about 120 fields
#define DEV_MEM_FULL (-1) // returned in place of M's code: every slot is taken (nothing was allocated)
enum DevMemKind { DEV_MEM_DEVICE = 0, DEV_MEM_PINNED = 1 };

struct DevMemOwner {
    void** field[DEV_MEM_SLOTS];
    unsigned char kind[DEV_MEM_SLOTS];
    int count;
};

template <class M> inline void dev_mem_free(DevMemKind kind, void* p) { kind == DEV_MEM_PINNED ? M::free_pinned(p) : M::free_device(p); }

// the one allocation of a field that is null: registered first, so that nothing can be allocated that release_all would not find
template <class M> inline int dev_mem_alloc(DevMemOwner* o, void** field, size_t bytes, DevMemKind kind)
{
    int i = 0;
    while (i < o->count && o->field[i] != field) i++;
    if (i == DEV_MEM_SLOTS) return DEV_MEM_FULL;
    if (i == o->count) { o->field[i] = field; o->kind[i] = (unsigned char)kind; o->count++; }
    const int rc = kind == DEV_MEM_PINNED ? M::alloc_pinned(field, bytes) : M::alloc_device(field, bytes);
    if (rc != 0) *field = nullptr;
    return rc;
}

// A buffer of a fixed size, allocated by whoever needs it first: a field that is set costs no call, otherwise exactly one
// allocation; on failure the field stays null.
template <class M, class T> inline int dev_mem_once(DevMemOwner* o, T** field, size_t bytes, DevMemKind kind = DEV_MEM_DEVICE)
{
    return *field ? 0 : dev_mem_alloc<M>(o, reinterpret_cast<void**>(field), bytes, kind);
}

// A buffer that grows with the largest size asked for.  *cap and need count elements of elem_bytes.  *cap >= need costs no call;
// otherwise the old block is freed and one new one allocated.  On failure the field is null and *cap 0.
template <class M, class T> inline int dev_mem_grow(DevMemOwner* o, T** field, size_t* cap, size_t need, size_t elem_bytes, DevMemKind kind = DEV_MEM_DEVICE)
{
    if (*cap >= need) return 0;
    if (*field) dev_mem_free<M>(kind, *field);
    *field = nullptr;
    *cap = 0;
    const int rc = dev_mem_alloc<M>(o, reinterpret_cast<void**>(field), need * elem_bytes, kind);
    if (rc == 0) *cap = need;
    return rc;
}

template <class M, class T> inline int dev_mem_once_pinned(DevMemOwner* o, T** field, size_t bytes) { return dev_mem_once<M>(o, field, bytes, DEV_MEM_PINNED); }
template <class M, class T> inline int dev_mem_grow_pinned(DevMemOwner* o, T** field, size_t* cap, size_t need, size_t elem) { return dev_mem_grow<M>(o, field, cap, need, elem, DEV_MEM_PINNED); }

// gives one buffer back early (a set of buffers that is only valid as a whole); the field stays registered
template <class M, class T> inline void dev_mem_release(DevMemOwner* o, T** field)
{
    for (int i = 0; i < o->count; i++)
        if (o->field[i] == reinterpret_cast<void**>(field) && *field) { dev_mem_free<M>((DevMemKind)o->kind[i], *field); *field = nullptr; }
}

// every registered field that is set: freed by its kind's function, then null.  The capacities are the caller's (a handle is deleted behind this).
template <class M> inline void dev_mem_release_all(DevMemOwner* o)
{
    for (int i = 0; i < o->count; i++)
        if (*o->field[i]) { dev_mem_free<M>((DevMemKind)o->kind[i], *o->field[i]); *o->field[i] = nullptr; }
}
