// Host memory check of csrc/resample.hip's argument checking: a stand-alone program (own main) that drives the entry points
// through every refusal that needs no device - null pointers, bad R / slots / parity / mask / n_in / positions / rate pairs.
// Build the host side with sanitizers and run it on the CPU; nothing here launches a kernel:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         tools/resample_args_check.cpp csm-train-pytorch_amd/csrc/resample.hip csm-train-pytorch_amd/csrc/csm_api.cpp -o resample_args_check
// Exit code 0 and "ok" = every call was refused (return 1) or, for N = 0, accepted with nothing to do - and no sanitizer report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "csm_hip.h"

static int fails = 0;
#define EXPECT(call, want)                                                                      \
    do {                                                                                        \
        const int rc__ = (call);                                                                \
        if (rc__ != (want)) { std::printf("FAIL %s -> %d (want %d): %s\n", #call, rc__, want, csm_last_error()); ++fails; } \
    } while (0)

struct Rows {
    int R = 2, n_slots = 4, max_in = 8, o = 2, n = 3, width = 7;
    long long ldy = 64;
    unsigned mask = 0;
    std::vector<int> slots{0, 1}, parity{0, 0}, n_in{4, 4};
    std::vector<long long> pos{0, 0};
    std::vector<const float*> x{nullptr, nullptr};
    float dummy = 0.f;                      // a non-null host address: the checks must refuse before anything reads it
    Rows() { x[0] = x[1] = &dummy; }
    int call() const {
        return csm_resample_stream_rows_f32(nullptr, x.data(), nullptr, nullptr, ldy, R, slots.data(), parity.data(), n_in.data(),
                                            pos.data(), mask, n_slots, max_in, o, n, width, nullptr);
    }
};

int main() {
    { Rows r; r.R = 0; EXPECT(r.call(), 1); }
    { Rows r; r.R = 17; EXPECT(r.call(), 1); }                      // (refused before the 2-entry arrays are walked)
    { Rows r; r.R = -3; EXPECT(r.call(), 1); }
    { Rows r; r.slots = {0, 4}; EXPECT(r.call(), 1); }
    { Rows r; r.slots = {-1, 0}; EXPECT(r.call(), 1); }
    { Rows r; r.slots = {1, 1}; EXPECT(r.call(), 1); }
    { Rows r; r.parity = {0, 2}; EXPECT(r.call(), 1); }
    { Rows r; r.parity = {-1, 0}; EXPECT(r.call(), 1); }
    { Rows r; r.mask = 4u; EXPECT(r.call(), 1); }
    { Rows r; r.mask = 0x80000000u; EXPECT(r.call(), 1); }
    { Rows r; r.n_in = {4, 9}; EXPECT(r.call(), 1); }
    { Rows r; r.n_in = {4, 0}; EXPECT(r.call(), 1); }
    { Rows r; r.n_in = {4, -1}; r.mask = 2u; EXPECT(r.call(), 1); }
    { Rows r; r.pos = {0, -1}; EXPECT(r.call(), 1); }
    { Rows r; r.pos = {0, 1LL << 62}; EXPECT(r.call(), 1); }
    { Rows r; r.ldy = 2; EXPECT(r.call(), 1); }
    { Rows r; r.n_slots = 0; EXPECT(r.call(), 1); }
    { Rows r; r.max_in = 0; EXPECT(r.call(), 1); }
    { Rows r; r.x[1] = nullptr; EXPECT(r.call(), 1); }
    { Rows r; r.o = 3; r.n = 3; EXPECT(r.call(), 1); }
    { Rows r; r.o = 4; r.n = 6; EXPECT(r.call(), 1); }
    { Rows r; r.o = 0; EXPECT(r.call(), 1); }
    { Rows r; r.width = 0; EXPECT(r.call(), 1); }
    { Rows r; r.o = 44101; r.n = 24000; r.width = 12; EXPECT(r.call(), 1); }
    { Rows r; r.o = 1999; r.n = 4001; r.width = 12; EXPECT(r.call(), 1); }
    { Rows r; r.o = 2147483647; r.n = 2; r.width = 2147483647; EXPECT(r.call(), 1); }
    { Rows r; EXPECT(r.call(), 1); }                                // all lists fine: refused at the null arena / table
    { Rows r; EXPECT(csm_resample_stream_rows_f32(nullptr, nullptr, nullptr, nullptr, 64, 2, nullptr, nullptr, nullptr, nullptr, 0, 4, 8,
                                                  2, 3, 7, nullptr), 1); }
    EXPECT(csm_resample_stream_f32(nullptr, 2, nullptr, 4, 0, 0, nullptr, nullptr, 64, 8, 2, 3, 7, nullptr), 1);
    EXPECT(csm_resample_stream_f32(nullptr, 0, nullptr, 4, 0, 0, nullptr, nullptr, 64, 8, 2, 3, 7, nullptr), 1);
    EXPECT(csm_resample_stream_f32(nullptr, 0, nullptr, 0, 0, 1, nullptr, nullptr, 0, 8, 2, 3, 7, nullptr), 1);
    EXPECT(csm_resample_f32(nullptr, nullptr, nullptr, 1, 16, 3, 3, 7, nullptr), 1);
    EXPECT(csm_resample_f32(nullptr, nullptr, nullptr, 0, 16, 2, 3, 7, nullptr), 1);
    EXPECT(csm_resample_f32(nullptr, nullptr, nullptr, 1, -1, 2, 3, 7, nullptr), 1);
    EXPECT(csm_resample_f32(nullptr, nullptr, nullptr, 1, 1LL << 40, 2, 3, 7, nullptr), 1);
    EXPECT(csm_resample_f32(nullptr, nullptr, nullptr, 1, 16, 2, 3, 7, nullptr), 1);
    EXPECT(csm_resample_f32(nullptr, nullptr, nullptr, 1, 0, 2, 3, 7, nullptr), 0);
    std::printf(fails ? "%d FAILED\n" : "ok (%d)\n", fails);
    return fails ? 1 : 0;
}
