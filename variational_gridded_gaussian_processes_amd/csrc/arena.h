// Two-pass workspace carver of every device workspace of the library.  A `layout` asks for its buffers with take() in a
// fixed order and is called twice: first to measure (take() hands out null), then, once the memory is there, to receive 256-byte-
// aligned slices of it.  The pieces below are the steps every site goes through -- measure, check the free memory, allocate, zero,
// place -- so that a site keeps its own order of releasing the old workspace and its own out-of-memory text.
#pragma once
#include "common.h"

#define VG_ARENA_SLACK 4096       // bytes allocated beyond what the layout takes

struct VgArena {
    char* base = nullptr;         // null: measuring pass
    size_t off = 0;
    template <typename T = double>
    T* take(size_t count) {
        off = (off + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

// bytes to allocate for `layout` (measuring pass)
template <class Layout>
static size_t vg_arena_measure(Layout&& layout) {
    VgArena a;
    layout(a);
    return a.off + VG_ARENA_SLACK;
}
// false: the device has fewer than `need` bytes free (*free_b of them); the caller says what does not fit
static inline bool vg_arena_fits(size_t need, size_t* free_b) {
    size_t total_b = 0;
    *free_b = 0;
    return !(hipMemGetInfo(free_b, &total_b) == hipSuccess && need > *free_b);
}
// placing pass over `mem`, whose first zero_bytes are cleared before; *used: what the layout took
template <class Layout>
static int vg_arena_place(void* mem, size_t zero_bytes, Layout&& layout, size_t* used = nullptr) {
    if (zero_bytes) VG_HIP(hipMemset(mem, 0, zero_bytes));
    VgArena a;
    a.base = reinterpret_cast<char*>(mem);
    layout(a);
    if (used) *used = a.off;
    return VGGP_OK;
}
// exact-size workspace: `bytes` (vg_arena_measure) of fresh, zeroed device memory, placed
template <class Layout>
static int vg_arena_alloc(void** mem, size_t bytes, Layout&& layout) {
    VG_HIP(hipMalloc(mem, bytes));
    return vg_arena_place(*mem, bytes, layout);
}
// grow-only workspace, not zeroed.  *grew: the arena was too small and has been replaced, so whatever it kept is gone.  oom: a format
// with two %.1f (GiB needed, GiB free) for the VGGP_ENOMEM raised when the device has less free memory than the arena needs; null: no
// such check, a failing hipMalloc speaks for itself.
template <class Layout>
static int vg_arena_carve(void** mem, size_t* bytes, const char* oom, bool* grew, Layout&& layout, size_t* used = nullptr) {
    const size_t need = vg_arena_measure(layout);
    *grew = *bytes < need;
    if (*grew) {
        if (*mem) { VG_HIP(hipFree(*mem)); *mem = nullptr; *bytes = 0; }
        size_t free_b = 0;
        if (oom && !vg_arena_fits(need, &free_b)) {
            vg_set_error(oom, (double)need / 1073741824.0, (double)free_b / 1073741824.0);
            return VGGP_ENOMEM;
        }
        VG_HIP(hipMalloc(mem, need));
        *bytes = need;
    }
    return vg_arena_place(*mem, 0, layout, used);
}
