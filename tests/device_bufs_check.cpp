// Host check of tsc::DeviceBufsT's bookkeeping (csrc/tsc_common.h) over a stub allocator: built with
// AddressSanitizer and UBSan on the host and run by tests/test_device_bufs_host.py.  No device, nothing loaded into Python.  A leak or a
// double free is the sanitizer's to report; the counts below catch what it cannot see (a buffer that is freed but still listed).
#include "../deeprl_signal_control_amd/csrc/tsc_common.h"

#include <cstdlib>
#include <set>

namespace {

struct StubMem {
    static std::set<void *> &live() { static std::set<void *> s; return s; }
    static int &copies_until_failure() { static int n = -1; return n; }       // 1: the next copy fails; < 0: none does
    static hipError_t malloc(void **p, size_t bytes) { *p = std::malloc(bytes); live().insert(*p); return hipSuccess; }
    static hipError_t zero(void *p, size_t bytes) { memset(p, 0, bytes); return hipSuccess; }
    static hipError_t copy(void *dst, const void *src, size_t bytes) {
        if (copies_until_failure() > 0 && --copies_until_failure() == 0) return hipErrorInvalidValue;
        memcpy(dst, src, bytes);
        return hipSuccess;
    }
    static void free(void *p) {
        if (!live().erase(p)) { fprintf(stderr, "free of a pointer that is not live\n"); abort(); }
        std::free(p);
    }
};

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

}  // namespace

int main() {
    const int src[4] = {1, 2, 3, 4};
    {
        tsc::DeviceBufsT<StubMem> bufs;
        const int *a = nullptr, *c = nullptr, *empty = nullptr;       // const fields, as most of EnvDev's are
        int *b = nullptr, *failed = nullptr;
        double *z = nullptr;
        // 1. uploads and allocations that succeed
        CHECK(bufs.upload(&a, src, 4) == hipSuccess && a[3] == 4);
        CHECK(bufs.upload(&b, src, 2) == hipSuccess && b[1] == 2);
        CHECK(bufs.upload(&c, src, 3) == hipSuccess && c[2] == 3);
        CHECK(bufs.upload(&empty, (const int *)nullptr, 0) == hipSuccess && empty);      // one element, nothing copied
        CHECK(bufs.alloc(&z, 3, true) == hipSuccess && z[0] == 0.0 && z[2] == 0.0);
        CHECK(bufs.owned.size() == 5 && StubMem::live().size() == 5);
        // 2. the second copy from here fails: its buffer is freed at once, the field untouched, the others as they were
        StubMem::copies_until_failure() = 2;
        int *ok = nullptr;
        CHECK(bufs.upload(&ok, src, 4) == hipSuccess);
        CHECK(bufs.upload(&failed, src, 4) == hipErrorInvalidValue && !failed);
        CHECK(bufs.owned.size() == 6 && StubMem::live().size() == 6 && a[0] == 1);
        // 3. release of a middle element
        bufs.release(b);
        CHECK(bufs.owned.size() == 5 && StubMem::live().size() == 5 && !StubMem::live().count(b) && a[0] == 1 && c[0] == 1);
        // 4. release of null and of a pointer that is not ours (twice the same: b is gone)
        int other = 0;
        bufs.release(nullptr); bufs.release(&other); bufs.release(b);
        CHECK(bufs.owned.size() == 5 && StubMem::live().size() == 5);
    }   // 5. destruction frees the rest
    CHECK(StubMem::live().empty());
    printf("device_bufs_check ok\n");
    return 0;
}
