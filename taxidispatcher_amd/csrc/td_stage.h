// td_stage.h — the host code between the C ABI and the kernels, one definition each: host copies of small inputs, the
// ragged-offset check, the result block of a batched call, layouts that size themselves (Carve) and the LDS budget.
// Carve and ragged_check need no HIP runtime (TD_STAGE_HOST_ONLY leaves the rest out: tests/stage_host_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "taxidispatcher_amd.h"

namespace td {

// A block laid out array after array: take<T>(count) is the next `count` elements, aligned to alignof(T) and no coarser, so
// consecutive arrays of one type are adjacent.  A layout is a function of a Carve&; run on a null base it yields the
// block's size (`at`) and each array's offset as its pointer, run on the allocation it sets the pointers.
struct Carve {
    uintptr_t base;
    size_t at = 0;
    explicit Carve(void *b = nullptr) : base((uintptr_t)b) {}
    template <class T>
    T *take(size_t count)
    {
        at = (at + alignof(T) - 1) & ~(alignof(T) - 1);
        T *r = (T *)(base + at);
#ifdef TD_CARVE_TRACE   // tests/stage_host_main.cpp records every array
        TD_CARVE_TRACE(at, sizeof(T) * count, alignof(T));
#endif
        at += sizeof(T) * count;
        return r;
    }
};

struct Ragged {
    int longest = 0, total = 0;
};

// offsets h[0 .. count] of `count` segments: they start at 0 and never decrease.  seg(b, length) is the caller's own refusal
// for model / world b, tested before b's "decreases" (its "more than n", or td_simb_create's cab count, which its loop
// tested first: the order of refusals stays the caller's); non-zero refuses.  report: td::fail.
template <class Seg = int (*)(int, int)>
int ragged_check(int (*report)(int, const char *, ...), const char *fn, const char *what, const char *noun, const int32_t *h, int count,
                 Ragged *r, Seg seg = +[](int, int) { return 0; })
{
    *r = Ragged{};
    if (h[0] != 0) return report(TD_EINVAL, "%s: %s[0] = %d, not 0", fn, what, h[0]);
    for (int b = 0; b < count; b++) {
        const int m = h[b + 1] - h[b];
        if (int rc = seg(b, m)) return rc;
        if (m < 0) return report(TD_EINVAL, "%s: %s decreases at %s %d (%d -> %d)", fn, what, noun, b, h[b], h[b + 1]);
        r->longest = std::max(r->longest, m);
    }
    r->total = h[count];
    return TD_OK;
}

}  // namespace td

#ifndef TD_STAGE_HOST_ONLY
#include <vector>

#include "td_common.h"

namespace td {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// b holds what `layout` lays out; the layout is run once for the size and once on the allocation
template <class L>
int carve_buf(Buf &b, L layout)
{
    Carve size;
    layout(size);
    int rc = ensure(b, size.at);
    if (rc) return rc;
    Carve c(b.p);
    layout(c);
    return TD_OK;
}

// host copies of n int32 values each (host or device source; a null source is left out): the copies from the device are
// queued one behind the other and the stream is synchronised once
struct HostCopy {
    const int32_t *src;
    size_t n;
    std::vector<int32_t> *h;
};
int host_copy(std::initializer_list<HostCopy> list);
inline int host_copy(const int32_t *src, size_t n, std::vector<int32_t> &h) { return host_copy({{src, n, &h}}); }

// dynamic LDS one workgroup may take (gfx950: 160 KiB per CU, all of it for one workgroup), less the static arrays (td_match.hip)
size_t lds_budget();

template <class K>
void lds_allow(K kernel, size_t shm)
{
    if (shm > 64 * 1024) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
}

// one output array of a batched call: the caller's device pointer, or a slice of the call's result block (a grow-only Buf)
// that is copied to the caller's host array at the end
struct Out {
    void *user;
    size_t bytes, off;
    void *dev_ptr;
    bool dev;
    void *dptr() const { return dev_ptr; }
};

// lays the host destinations out in `buf`, the error word behind them (*d_err, zeroed on the stream)
int outputs_prepare(Buf &buf, Out *o, int k, int **d_err);
// queues the copies of the host destinations (to the caller's arrays, or to bounce + off where bounce is non-null) and of the
// error word, synchronises the stream; *e = the error word
int outputs_fetch(const Out *o, int k, const int *d_err, char *bounce, int *e);

// the end of a call that writes its host destinations whatever comes of it; decode(error word) is the return code
template <class D>
int outputs_finish(const Out *o, int k, const int *d_err, D decode)
{
    int e;
    int rc = outputs_fetch(o, k, d_err, nullptr, &e);
    return rc ? rc : decode(e);
}

// the end of a call whose host destinations are written only when it succeeded: they land in `bounce` first
template <class D>
int outputs_finish_on_success(const Out *o, int k, const int *d_err, std::vector<char> &bounce, D decode)
{
    size_t need = 0;
    for (int i = 0; i < k; i++)
        if (o[i].user && !o[i].dev) need = std::max(need, o[i].off + o[i].bytes);
    bounce.resize(need);
    int e;
    int rc = outputs_fetch(o, k, d_err, bounce.data(), &e);
    if (rc || (rc = decode(e))) return rc;
    for (int i = 0; i < k; i++)
        if (o[i].user && !o[i].dev && o[i].bytes) memcpy(o[i].user, bounce.data() + o[i].off, o[i].bytes);
    return TD_OK;
}

}  // namespace td
#endif
