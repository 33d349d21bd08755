// conv3p_host.hpp -- host-only helpers shared by conv3p_abi.hip and the conv3p_abi_*.hpp files it includes.
#pragma once
#include "../../include/conv3p.h"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace {

constexpr size_t kAlign = 256;
inline size_t up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

inline int hip_ok()
{
    return hipGetLastError() == hipSuccess ? CONV3P_OK : CONV3P_ERR_LAUNCH;
}

#define TRY(expr) do { int rc_ = (expr); if (rc_ != CONV3P_OK) return rc_; } while (0)

inline int buf_check(const void *p, size_t have, size_t need)
{
    if (need == 0) return CONV3P_OK;
    if (!p || (reinterpret_cast<uintptr_t>(p) % kAlign) != 0 || have < need) return CONV3P_ERR_WORKSPACE;
    return CONV3P_OK;
}

// grid of a launch over `work` workgroups' worth of items, at most `cap`
inline unsigned capped_grid(size_t work, size_t cap) { return (unsigned)(work < cap ? work : cap); }

// A workspace layout, written once: a sequence of take()s over `base`.  Every array starts kAlign-aligned.  With a null
// base the same walk only measures: the pointers are null and bytes() is the size the workspace must have.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *b) : base(static_cast<char *>(b)) {}
    template <typename T> T *take(size_t count)
    {
        T *r = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += up(count * sizeof(T));
        return r;
    }
    size_t bytes() const { return off; }
};
// ... of a single array
template <typename T> inline size_t carve_one(void *ws, size_t count, T *&p)
{
    Carver cv(ws);
    p = cv.take<T>(count);
    return cv.bytes();
}

}  // namespace
