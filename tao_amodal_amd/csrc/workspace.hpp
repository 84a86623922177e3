// Caller-allocated scratch buffers.  Every workspace has ONE layout function:
// it take()s the stage's tables from a Carve in buffer order.  taoamd_*_workspace()
// is measure() of it; the entry point runs it on the caller's pointer and
// refuses the call unless fits().  No byte count is written down anywhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace taoamd {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carve {
    unsigned char *base;   // the caller's pointer rounded up to 256; null: measuring only
    size_t used = 0;       // bytes of the pieces taken so far
    explicit Carve(void *workspace)
        : base((unsigned char *)align256((uintptr_t)workspace)) {}
    // the next 256-aligned piece (null when measuring)
    template <class T> T *take(size_t count)
    {
        T *p = base ? (T *)(base + used) : nullptr;
        used += align256(count * sizeof(T));
        return p;
    }
    // p + i inside one piece (null stays null)
    template <class T> static T *at(T *p, size_t i) { return p ? p + i : nullptr; }
    // the pieces + what rounding the caller's pointer up may cost
    size_t bytes() const { return used + 256; }
    // the caller passed the size it was told (whatever its pointer's alignment),
    // and the last piece ends inside what it passed
    bool fits(const void *workspace, size_t workspace_bytes) const
    {
        return workspace_bytes >= bytes() &&
               (size_t)(base - (const unsigned char *)workspace) + used <= workspace_bytes;
    }
};

// bytes() of a layout, layout(Carve &), run without a buffer
template <class F> size_t measure(F layout)
{
    Carve c(nullptr);
    layout(c);
    return c.bytes();
}

}  // namespace taoamd
