// io_ceiling.hip -- what does the MEMORY SYSTEM allow for the headline kernel's traffic, with the arithmetic taken out?
// Same shape as minsnap_fixed_persistent_kernel<4,16>: 2 x CU persistent workgroups of 128 threads walk 64-trajectory
// slices (and, for comparison, 4 / 8 / 16 workgroups per CU: more waves = more bytes in flight than the solver can have); per slice a workgroup reads the slice's 34 816 B of inputs (16 B per lane, coalesced) and writes its 196 608 B
// of coefficients -- either in the kernel's own store shape (one wave instruction = 4 trajectory rows x 256 contiguous
// bytes, rows 3072 B apart: "rows") or as fully contiguous 1 KB per wave instruction ("linear").  The written values
// depend on what was read, so nothing is optimised away.
//   hipcc --offload-arch=gfx950 -O3 tools/io_ceiling.hip -o /tmp/io_ceiling && /tmp/io_ceiling
//
// `io_ceiling --policy [rounds]`: the store-policy sweep.  The solver's exact order-4 store sequence
// (per segment pair a burst of 8 rows x 128 B, then two bursts of 4 rows x 256 B; every byte of the slice written once) at
// two workgroups per CU, B = 65536 and 524288, for each cache policy of the 16-byte store: plain and nt as global stores,
// and plain / sc1 / sc0 sc1 / sc1 nt as buffer stores through a per-slice descriptor (the buffer form carries the cache
// bits in its aux operand).  Every (B, policy) is timed `rounds` times (default 3), interleaved, so the spread of a
// policy across rounds is the session's run-to-run spread.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef double v2d_t __attribute__((ext_vector_type(2)));

// NT: the stores carry the non-temporal bit (what the solver does for launches beyond the Infinity Cache)
template <bool ROWS, bool NT>
__global__ void __launch_bounds__(128) io_kernel(const double2 *in, double2 *out, int n_slices) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = blockIdx.x; s < n_slices; s += gridDim.x) {
        const double2 *src = in + (size_t)s * (34816 / 16);
        double2 acc = make_double2(0.0, 0.0);
        for (int i = tid; i < 34816 / 16; i += 128) { const double2 v = src[i]; acc.x += v.x; acc.y += v.y; }
        char *dst = (char *)out + (size_t)s * 196608;
        // each wave writes half of the slice: 96 wave-instructions of 1 KB
        for (int k = 0; k < 96; ++k) {
            size_t off;
            if (ROWS) {
                // instruction k of wave w: segment pair q = k / 12 (of 8 per half... 8 pairs x 12 instructions), rows 4*(k%12.. ) -- 16 row groups x 6 pieces
                const int pair = (k / 16) + wave * 4 + (k / 16 >= 4 ? 0 : 0);   // 6 pairs per wave half: k/16 in 0..5
                const int rowgrp = k % 16;                                        // 16 groups of 4 trajectories
                off = (size_t)(rowgrp * 4 + (lane >> 4)) * 3072 + (size_t)((pair % 8) * 384) + (size_t)(lane & 15) * 16;
            } else {
                off = (size_t)(wave * 96 + k) * 1024 + (size_t)lane * 16;
            }
            acc.x += 1.0;
            if (NT) { v2d_t x = {acc.x, acc.y}; __builtin_nontemporal_store(x, reinterpret_cast<v2d_t *>(dst + off)); }
            else *reinterpret_cast<double2 *>(dst + off) = acc;
        }
    }
}

// AUX < 0: global store (-1 plain, -2 nt); AUX >= 0: buffer store with that aux operand (0 plain, 2 nt, 16 sc1, 17 sc0 sc1,
// 18 sc1 nt).  One wave writes the segment pairs of its half of the slice.
typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
template <int AUX>
__global__ void __launch_bounds__(128) io_policy_kernel(const double2 *in, double2 *out, int n_slices) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned o8 = (unsigned)((lane >> 3) * 3072 + (lane & 7) * 16), o16 = (unsigned)((lane >> 4) * 3072 + (lane & 15) * 16);
    for (int s = blockIdx.x; s < n_slices; s += gridDim.x) {
        const double2 *src = in + (size_t)s * (34816 / 16);
        double2 acc = make_double2(0.0, 0.0);
        for (int i = tid; i < 34816 / 16; i += 128) { const double2 v = src[i]; acc.x += v.x; acc.y += v.y; }
        char *dst = (char *)out + (size_t)s * 196608;   // wave-uniform
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(dst, 0, 196608, 0x00020000);
#pragma unroll
        for (int pair = 0; pair < 4; ++pair) {
#pragma unroll
            for (int j = 0; j < 24; ++j) {
                // j < 8: 8 rows x the 128 bytes that complete the pair's last line; else 4 rows x its first 256 bytes
                const unsigned disp = (unsigned)((wave * 4 + pair) * 384 + (j < 8 ? 256 + j * 8 * 3072 : (j - 8) * 4 * 3072));
                const unsigned voff = j < 8 ? o8 : o16;
                acc.x += 1.0;
                if constexpr (AUX >= 0) {
                    const unsigned long long lo = __builtin_bit_cast(unsigned long long, acc.x), hi = __builtin_bit_cast(unsigned long long, acc.y);
                    const v4u_t x = {(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
                    __builtin_amdgcn_raw_buffer_store_b128(x, rsrc, (int)voff, (int)disp, AUX);
                } else if constexpr (AUX == -2) {
                    v2d_t x = {acc.x, acc.y};
                    __builtin_nontemporal_store(x, reinterpret_cast<v2d_t *>(dst + disp + voff));
                } else {
                    *reinterpret_cast<double2 *>(dst + disp + voff) = acc;
                }
            }
        }
    }
}

static int policy_sweep(int rounds) {
    const int Bs[2] = {65536, 524288};
    const size_t max_slices = 524288 / 64;
    double2 *in, *out;
    if (hipMalloc(&in, max_slices * 34816) != hipSuccess || hipMalloc(&out, max_slices * 196608) != hipSuccess) return 1;
    hipMemset(in, 0, max_slices * 34816);
    hipDeviceProp_t p;
    hipGetDeviceProperties(&p, 0);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    struct { const char *name; void (*k)(const double2 *, double2 *, int); } pol[] = {
        {"global plain", io_policy_kernel<-1>}, {"global nt", io_policy_kernel<-2>}, {"buffer plain", io_policy_kernel<0>},
        {"buffer sc1", io_policy_kernel<16>},   {"buffer sc0 sc1", io_policy_kernel<17>}, {"buffer sc1 nt", io_policy_kernel<18>}};
    const int grid = 2 * p.multiProcessorCount;
    for (int round = 0; round < rounds; ++round)
    for (int bi = 0; bi < 2; ++bi)
    for (auto &q : pol) {
        const int n_slices = Bs[bi] / 64;
        for (int w = 0; w < 3; ++w) hipLaunchKernelGGL(q.k, dim3(grid), dim3(128), 0, 0, in, out, n_slices);
        hipEventRecord(e0, 0);
        const int reps = 20;
        for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(q.k, dim3(grid), dim3(128), 0, 0, in, out, n_slices);
        hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) return 1;
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        ms /= reps;
        const double bytes = (double)n_slices * (34816.0 + 196608.0);
        std::printf("{\"round\": %d, \"policy\": \"%s\", \"workgroups_per_cu\": 2, \"store_shape\": \"order-4 pairs (8 x 128 B, 2 x 4 x 256 B)\", \"B\": %d, \"us\": %.2f, \"TBps\": %.3f}\n",
                    round, q.name, Bs[bi], ms * 1e3, bytes / (ms * 1e-3) / 1e12);
        std::fflush(stdout);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--policy")) return policy_sweep(argc > 2 ? std::atoi(argv[2]) : 3);
    const int B = 524288, n_slices = B / 64;
    double2 *in, *out;
    hipMalloc(&in, (size_t)n_slices * 34816);
    hipMalloc(&out, (size_t)n_slices * 196608);
    hipMemset(in, 0, (size_t)n_slices * 34816);
    hipDeviceProp_t p;
    hipGetDeviceProperties(&p, 0);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int nt = 0; nt < 2; ++nt)
    for (int per_cu = 2; per_cu <= 8; per_cu *= 2)
    for (int mode = 0; mode < 2; ++mode) {
        const int grid = per_cu * p.multiProcessorCount;
        auto launch = [&] {
            if (mode) { if (nt) hipLaunchKernelGGL((io_kernel<true, true>), dim3(grid), dim3(128), 0, 0, in, out, n_slices);
                        else hipLaunchKernelGGL((io_kernel<true, false>), dim3(grid), dim3(128), 0, 0, in, out, n_slices); }
            else { if (nt) hipLaunchKernelGGL((io_kernel<false, true>), dim3(grid), dim3(128), 0, 0, in, out, n_slices);
                   else hipLaunchKernelGGL((io_kernel<false, false>), dim3(grid), dim3(128), 0, 0, in, out, n_slices); }
        };
        for (int w = 0; w < 3; ++w) launch();
        hipEventRecord(e0, 0);
        const int reps = 20;
        for (int r = 0; r < reps; ++r) launch();
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        ms /= reps;
        const double bytes = (double)n_slices * (34816.0 + 196608.0);
        std::printf("{\"nt_stores\": %d, \"workgroups_per_cu\": %d, \"store_shape\": \"%s\", \"B\": %d, \"us\": %.1f, \"TBps\": %.3f, \"frac_of_8TBps\": %.3f}\n", nt, per_cu, mode ? "rows (4 x 256 B per wave instruction)" : "linear (1 KB per wave instruction)",
                    B, ms * 1e3, bytes / (ms * 1e-3) / 1e12, bytes / (ms * 1e-3) / 8e12);
    }
    return 0;
}
