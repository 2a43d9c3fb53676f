// search_edlib.cpp -- the CPU yardstick of tools/search_bench.py: edlib's HW / SHW modes with EDLIB_TASK_LOC over a pool of
// pairs on `threads` host threads, timed inside one call (no interpreter in the loop).  edlib itself is not linked: the
// caller passes the path of the shared library (oracle/_ref/libedlib_ref.so) and the two entry points are taken with
// dlsym; the two structs below restate edlib.h's public layout.  Built by the tool into tools/bin/.
#include <dlfcn.h>
#include <stdint.h>

#include <chrono>
#include <thread>
#include <vector>

struct AlignConfig { int k, mode, task; const void* additionalEqualities; int additionalEqualitiesLength; };
struct AlignResult { int status, editDistance; int* endLocations; int* startLocations; int numLocations; unsigned char* alignment; int alignmentLength, alphabetLength; };
typedef AlignResult (*align_fn)(const char*, int, const char*, int, AlignConfig);
typedef void (*free_fn)(AlignResult);

// -> seconds, or -1 where the library cannot be loaded; out3[3 i ..] = {d, start, end} or {-1, -1, -1} = beyond the bound
extern "C" double search_edlib_run(const char* lib_path, int64_t n, const char* ppool, const int64_t* poff, const int32_t* plen,
                                   const char* tpool, const int64_t* toff, const int32_t* tlen, int mode, int bound, int threads, int32_t* out3) {
    void* h = dlopen(lib_path, RTLD_NOW | RTLD_LOCAL);
    if (!h) return -1;
    const align_fn align = (align_fn)dlsym(h, "edlibAlign");
    const free_fn release = (free_fn)dlsym(h, "edlibFreeAlignResult");
    if (!align || !release) return -1;
    const AlignConfig cfg{bound, mode, 1 /* EDLIB_TASK_LOC */, nullptr, 0};
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w)
        pool.emplace_back([&, w] {
            for (int64_t i = n * w / threads; i < n * (w + 1) / threads; ++i) {
                const AlignResult r = align(ppool + poff[i], plen[i], tpool + toff[i], tlen[i], cfg);
                int32_t* o = out3 + 3 * i;
                if (r.status == 0 && r.editDistance >= 0 && r.numLocations > 0) { o[0] = r.editDistance; o[1] = r.startLocations[0]; o[2] = r.endLocations[0] + 1; }
                else { o[0] = o[1] = o[2] = -1; }
                release(r);
            }
        });
    for (std::thread& t : pool) t.join();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
