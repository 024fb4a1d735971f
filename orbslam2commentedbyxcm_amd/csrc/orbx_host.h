// orbx_host.h -- host-side helpers shared by the ABI translation units: the error returns,
// the grow-only device buffer, the host calls' clock and the staging of the host forms.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_error.h"
#include "orbx_layout.h"

namespace orbx {

// for the handles that borrow a matcher's device and stream (orbx_matcher.cpp)
int matcher_device(const orbx_matcher* m);
hipStream_t matcher_stream(const orbx_matcher* m);
void matcher_set_last_call_us(orbx_matcher* m, double us);

inline int fail(int code, const char* what) {
    set_last_error(what ? what : "");
    return code;
}

inline int hip_fail(hipError_t e, const char* where) {
    set_last_error(std::string(where) + ": " + hipGetErrorString(e));
    return ORBX_ERR_HIP;
}

#define HIP_TRY(expr)                                            \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return orbx::hip_fail(_e, #expr);  \
    } while (0)

// Grow-only device allocation.  No destructor: the orbx_*_destroy entry points release()
// what they own, and nothing once unloading() is true (DESIGN.md §1 "Teardown").
struct DeviceBuffer {
    char* p = nullptr;
    size_t cap = 0;
    // Growing waits for the stream's work, which may still read the old allocation; a
    // failed hipMalloc leaves {nullptr, 0}.
    hipError_t reserve(size_t bytes, hipStream_t s) {
        if (bytes <= cap) return hipSuccess;
        hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess && p) e = hipFree(p);
        if (e != hipSuccess) return e;
        p = nullptr;
        cap = 0;
        e = hipMalloc((void**)&p, bytes);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Scoped: stores the enclosing host call's wall time (entry to return, errors included) in
// the matcher's last_call_us.
struct CallClock {
    orbx_matcher* m;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit CallClock(orbx_matcher* mm) : m(mm) {}
    ~CallClock() {
        if (m) matcher_set_last_call_us(m, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// Staging of a single host form (DESIGN.md §1 "Host forms").  Each array is declared once,
// with the field of the batch struct that takes its device address: n elements in use of
// cap reserved.  Uploads get a region each, in the order declared; results are packed into
// one block behind them.  stage() sizes the buffer, fills in the fields and issues the
// uploads in the order declared; download() is the one copy back of the result block, the
// one synchronise, and the scatter to the caller's arrays.
struct HostStage {
    struct Entry {
        void* field;        // where the device address goes
        const void* src;    // what to upload, or null
        const void* dst;    // results: the caller's field that holds the destination, or null
        size_t off, bytes;  // offset in the buffer (results: in the result block), bytes in use
        bool result, optional;
    };
    Layout buf, res{nullptr};
    std::vector<Entry> entries;
    std::vector<char> h;      // the downloaded result block
    char* results = nullptr;  // the result block on the device, once staged

    explicit HostStage(size_t (*round)(size_t)) : buf(round) {}

    // an upload; nothing is copied when n is 0
    template <class D>
    void in(D** field, const void* host, size_t n, size_t cap) {
        entries.push_back({field, host, nullptr, buf.take(cap * sizeof(D)), n * sizeof(D), false, false});
    }
    // an upload of an array that may be absent: a null host array gives a null device address
    template <class D>
    void in_optional(D** field, const void* host, size_t n, size_t cap) {
        entries.push_back({field, host, nullptr, buf.take(cap * sizeof(D)), n * sizeof(D), false, true});
    }
    // part of the result block; *host may be null (nothing is scattered).  Returns the
    // entry, for result().
    template <class D, class H>
    int out(D** field, H* const* host, size_t n, size_t cap) {
        static_assert(sizeof(D) == sizeof(H), "device and host element sizes differ");
        entries.push_back({field, nullptr, host, res.take(cap * sizeof(D)), n * sizeof(D), true, false});
        return (int)entries.size() - 1;
    }
    // an upload placed inside the result block
    template <class D, class H>
    void inout(D** field, H* const* host, size_t n, size_t cap) {
        entries[(size_t)out(field, host, n, cap)].src = *host;
    }

    hipError_t stage(DeviceBuffer& b, hipStream_t s) {
        const size_t res_off = buf.take(res.total());
        hipError_t e = b.reserve(buf.total(), s);
        if (e != hipSuccess) return e;
        results = b.p + res_off;
        for (const Entry& x : entries) {
            char* d = x.optional && !x.src ? nullptr : (x.result ? results : b.p) + x.off;
            std::memcpy(x.field, &d, sizeof(d));
            // pageable sources: staged by the runtime before each call returns
            if (x.src && x.bytes) e = hipMemcpyAsync(d, x.src, x.bytes, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    bool staged() const { return results != nullptr; }
    hipError_t zero_results(hipStream_t s) { return hipMemsetAsync(results, 0, res.total(), s); }
    // the result block up to the end of the last array's elements in use
    size_t results_in_use() const { return entries.back().off + entries.back().bytes; }

    hipError_t download(hipStream_t s, size_t bytes) {
        h.resize(bytes);
        hipError_t e = hipMemcpyAsync(h.data(), results, bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        for (const Entry& x : entries) {
            if (!x.dst) continue;
            void* to = nullptr;
            std::memcpy(&to, x.dst, sizeof(to));
            if (to && x.bytes) std::memcpy(to, h.data() + x.off, x.bytes);
        }
        return hipSuccess;
    }
    hipError_t download(hipStream_t s) { return download(s, res.total()); }
    // an entry's bytes in the downloaded block
    const char* result(int entry) const { return h.data() + entries[(size_t)entry].off; }
};

}  // namespace orbx
