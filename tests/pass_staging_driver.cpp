// Unit driver of vulkancomputeraytracing_amd/csrc/pass_staging.hpp (the staging of the host forms
// behind the C ABI), built and run on the CPU by tests/test_pass_staging_cpu.py with the address
// and undefined-behaviour sanitizers. The HIP calls the header makes are defined here over malloc,
// free and memcpy, counting calls; "device" memory is exactly sized heap memory, so a copy past
// count * elem is the sanitizer's to report. `fail_next` makes the next allocation fail. Prints
// one line per case: "<name> <numbers>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "pass_staging.hpp"

namespace {

struct Counts {
    int allocs = 0, frees = 0, uploads = 0, downloads = 0, syncs = 0;
};
Counts calls;
bool fail_next = false;
hipStream_t const kStream = reinterpret_cast<hipStream_t>(0x51);
bool other_stream = false;  // a call named another stream than the one given

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    calls.allocs++;
    if (fail_next) {
        fail_next = false;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    calls.frees++;
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                          hipStream_t stream) {
    (kind == hipMemcpyHostToDevice ? calls.uploads : calls.downloads)++;
    other_stream |= stream != kStream;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    calls.syncs++;
    other_stream |= stream != kStream;
    return hipSuccess;
}
}

namespace {

using vcrt::Plane;
using vcrt::Staging;
using vcrt::StagingPool;
using Bytes = std::vector<unsigned char>;

Counts take() { return std::exchange(calls, Counts{}); }
int hip_calls(const Counts& c) { return c.allocs + c.frees + c.uploads + c.downloads + c.syncs; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool all_are(const Bytes& b, unsigned char v) {
    for (unsigned char x : b)
        if (x != v) return false;
    return true;
}

// The device form: no HIP call in begin() or end(), the caller's pointers handed back.
void device_form() {
    StagingPool pool;
    Bytes a(64, 1), b(48, 2);
    take();
    Staging s(pool, kStream);
    const VkResult r = s.begin(false, 4, {vcrt::in4(reinterpret_cast<float*>(a.data())),
                                          Plane{b.data(), 12, true, true}, vcrt::in1(nullptr)});
    const VkResult e = s.end();
    std::printf("device_form %d %d %d %d %d %d\n", static_cast<int>(r), static_cast<int>(e),
                hip_calls(take()), s.at<unsigned char>(0) == a.data(),
                s.at<unsigned char>(1) == b.data(), s.at(2) == nullptr);
}

// The host form over an input, a plain output, a kept output (uploaded when `keep`) and a null
// optional plane: what begin() and end() call, what the device planes hold, what comes back.
void host_form(bool keep) {
    StagingPool pool;
    const size_t n = 5;
    Bytes in(n * 16, 0x11), out(n * 4, 0x22), kept(n * 16, 0x33);
    take();
    Staging s(pool, kStream);
    const VkResult r = s.begin(true, n, {Plane{in.data(), 16, false}, Plane{out.data(), 4, true},
                                        vcrt::in4(nullptr), Plane{kept.data(), 16, true, keep}});
    const Counts b = take();
    const bool in_up = std::memcmp(s.at<unsigned char>(0), in.data(), in.size()) == 0;
    const bool kept_up = std::memcmp(s.at<unsigned char>(3), kept.data(), kept.size()) == 0;
    // the run: the pass writes the plain output whole and the kept one in part
    std::memset(s.at<unsigned char>(1), 0x44, out.size());
    std::memset(s.at<unsigned char>(3), 0x55, 16);
    const VkResult e = s.end();
    const Counts c = take();
    std::printf("host_form_keep%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", keep ? 1 : 0,
                static_cast<int>(r), b.allocs, b.uploads, b.downloads, b.syncs, in_up, kept_up,
                s.at(2) == nullptr, static_cast<int>(e), c.uploads, c.downloads, c.syncs,
                all_are(out, 0x44), all_are(in, 0x11) && kept[0] == 0x55 && kept[15] == 0x55);
}

// No two planes of a call share memory: six planes of every element size, a pattern each, written
// through the staged pointers and read back; every staged pointer is 16-byte aligned and no copy
// goes past count * elem (the host planes and the stand-in device planes are exactly sized).
void element_sizes(size_t count) {
    StagingPool pool;
    const size_t elems[6] = {1, 2, 4, 12, 16, 32};
    Bytes host[6];
    for (int i = 0; i < 6; i++) host[i].assign(count * elems[i], static_cast<unsigned char>(i + 1));
    take();
    Staging s(pool, kStream);
    const VkResult r = s.begin(true, count, {Plane{host[0].data(), elems[0], true, true},
                                            Plane{host[1].data(), elems[1], true, true},
                                            Plane{host[2].data(), elems[2], true, true},
                                            Plane{host[3].data(), elems[3], true, true},
                                            Plane{host[4].data(), elems[4], true, true},
                                            Plane{host[5].data(), elems[5], true, true}});
    bool aligned = true, uploaded = true, distinct = true;
    for (int i = 0; i < 6; i++) {
        unsigned char* d = s.at<unsigned char>(i);
        aligned &= aligned16(d);
        for (size_t k = 0; k < host[i].size(); k++) uploaded &= d[k] == i + 1;
        std::memset(d, 0xa0 + i, host[i].size());
    }
    for (int i = 0; i < 6; i++)  // every pattern still stands after the others were written
        for (size_t k = 0; k < host[i].size(); k++)
            distinct &= s.at<unsigned char>(i)[k] == 0xa0 + i;
    const VkResult e = s.end();
    const Counts c = take();
    bool back = true;
    for (int i = 0; i < 6; i++) back &= all_are(host[i], static_cast<unsigned char>(0xa0 + i));
    std::printf("element_sizes_%zu %d %d %d %d %d %d %d %d %d %d\n", count, static_cast<int>(r),
                static_cast<int>(e), c.allocs, c.uploads, c.downloads, c.syncs, aligned, uploaded,
                distinct, back);
}

// One call of `count` float4 and 12-byte planes on a pool that lives on: the allocations it makes.
int allocs_of(StagingPool& pool, size_t count) {
    Bytes a(count * 16, 1), b(count * 12, 2), c(count * 16, 3);
    take();
    Staging s(pool, kStream);
    if (s.begin(true, count, {Plane{a.data(), 16, false}, Plane{b.data(), 12, false},
                              Plane{c.data(), 16, true}}) != VK_SUCCESS ||
        s.end() != VK_SUCCESS)
        std::abort();
    return take().allocs;
}

void large_small_large() {
    StagingPool pool;
    const int first = allocs_of(pool, 1000), second = allocs_of(pool, 3);
    std::printf("large_small_large %d %d %d\n", first, second, allocs_of(pool, 1000));
}

// One plane more than the pool holds, wide or narrow: refused, and nothing written or called.
void too_wide() {
    StagingPool pool;
    Bytes in(16, 7);
    const Plane w = Plane{in.data(), 16, false}, n = Plane{in.data(), 4, false};
    static_assert(sizeof(pool.wide) / sizeof(pool.wide[0]) == 8 &&
                      sizeof(pool.narrow) / sizeof(pool.narrow[0]) == 4,
                  "the lists below are one plane wider than the pool");
    take();
    Staging a(pool, kStream), b(pool, kStream), fits(pool, kStream);
    const VkResult rw = a.begin(true, 1, {w, w, w, w, w, w, w, w, w});
    const VkResult rn = b.begin(true, 1, {n, n, n, n, n});
    const int called = hip_calls(take());
    const VkResult rf = fits.begin(true, 1, {w, w, w, w, w, w, w, w, n, n, n, n});
    std::printf("too_wide %d %d %d %d %d\n", rw == VK_ERROR_UNKNOWN, rn == VK_ERROR_UNKNOWN,
                called, static_cast<int>(rf), take().allocs);
}

// No elements: nothing is allocated, copied or waited for, in either form.
void count_zero() {
    StagingPool pool;
    Bytes none(1);  // (a plane that is there, of no elements)
    int called = 0, ok = 1;
    for (bool host : {false, true}) {
        take();
        Staging s(pool, kStream);
        ok &= s.begin(host, 0, {Plane{none.data(), 12, false}, Plane{none.data(), 32, true, true},
                                Plane{none.data(), 1, true}}) == VK_SUCCESS;
        ok &= s.end() == VK_SUCCESS;
        called += hip_calls(take());
    }
    std::printf("count_zero %d %d\n", ok, called);
}

// The second of three allocations fails: the error comes back, and the next call succeeds.
void allocation_fails() {
    StagingPool pool;
    Bytes a(32, 1), b(32, 2), c(32, 3);
    auto call = [&](bool fail_second) {
        Staging s(pool, kStream);
        // (the first plane is narrow, so the wide list's first allocation is the call's second)
        const Plane first = Plane{a.data(), 4, false};
        if (fail_second) {
            Staging one(pool, kStream);
            if (one.begin(true, 8, {first}) != VK_SUCCESS) std::abort();
            fail_next = true;
        }
        VkResult r =
            s.begin(true, 2, {first, Plane{b.data(), 16, false}, Plane{c.data(), 16, true}});
        if (r == VK_SUCCESS) r = s.end();
        return r;
    };
    take();
    const VkResult failed = call(true);
    const Counts f = take();
    const VkResult next = call(false);
    const Counts n = take();
    std::printf("allocation_fails %d %d %d %d %d %d\n", failed == VK_ERROR_OUT_OF_DEVICE_MEMORY,
                f.downloads, f.syncs, static_cast<int>(next), n.allocs, n.downloads);
}

}  // namespace

int main() {
    device_form();
    host_form(false);
    host_form(true);
    element_sizes(1);
    element_sizes(7);  // 7, 14, 28, 84, 112 and 224 bytes: but for two, no multiple of 16
    large_small_large();
    too_wide();
    count_zero();
    allocation_fails();
    std::printf("streams %d\n", other_stream ? 1 : 0);
    return 0;
}
