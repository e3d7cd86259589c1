// Host program of tests/test_dev_buf_state.py: the state of a DevBuf (viprs_amd/csrc/dev_buf.h) around a failed allocation,
// with stand-in allocators -- no device, no HIP call except the hipFree of a null-free buffer that never happens here.
#include <cstdio>

#include "../viprs_amd/csrc/dev_buf.h"

static int calls = 0;
static char arena[4096];

static hipError_t refuse(void** q, size_t) { ++calls; *q = nullptr; return hipErrorOutOfMemory; }
static hipError_t grant(void** q, size_t bytes) { ++calls; *q = bytes <= sizeof(arena) ? arena : nullptr; return hipSuccess; }

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    viprs::DevBuf<char> b;
    // a failed allocation leaves the buffer empty: neither the pointer nor the capacity survives
    CHECK(b.reserve_with(1000, refuse) == hipErrorOutOfMemory && calls == 1);
    CHECK(b.p == nullptr && b.n == 0);
    // the retry with a smaller request (what the LD call's message recommends) allocates again: it is not skipped
    CHECK(b.reserve_with(100, grant) == hipSuccess && calls == 2);
    CHECK(b.p == arena && b.n == 100);
    // large enough: kept, the allocator is not asked
    CHECK(b.reserve_with(100, refuse) == hipSuccess && b.reserve_with(7, refuse) == hipSuccess && calls == 2);
    CHECK(b.p == arena && b.n == 100);
    b.p = nullptr;                                  // (the arena is not device memory: nothing to free)
    b.n = 100;
    // a capacity without a pointer vouches for nothing
    CHECK(b.reserve_with(50, grant) == hipSuccess && calls == 3 && b.p == arena && b.n == 50);
    b.p = nullptr;
    // growing and failing: empty again, and an allocator that "succeeds" with a null pointer counts as a failure
    CHECK(b.reserve_with(200, refuse) == hipErrorOutOfMemory && b.p == nullptr && b.n == 0);
    CHECK(b.reserve_with(1 << 20, grant) == hipErrorOutOfMemory && b.p == nullptr && b.n == 0);
    // nothing asked for: nothing allocated
    const int before = calls;
    CHECK(b.reserve_with(0, refuse) == hipSuccess && b.alloc_with(0, refuse) == hipSuccess && calls == before);
    CHECK(b.p == nullptr && b.n == 0);
    std::printf("dev_buf_state OK\n");
    return 0;
}
