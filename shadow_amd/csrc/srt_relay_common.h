// srt_relay_common.h -- what the packet stages' step headers (srt_*_step.h)
// share, written once for the host and the device: the saturating u64
// arithmetic of the reference's SimulationTime / token counts, the
// host-or-device updates of the call-wide words, the walk of a grouped batch
// (a host's segment, the late list's length, the scan's clamped base), and the
// relays' TokenBucket.  Plain host compilers build it for tests/asan: nothing
// HIP-only outside SRT_HD and __HIP_DEVICE_COMPILE__.
//
// Reference: src/main/network/relay/token_bucket.rs (lazy_refill,
// conforming_remove, compute_conforming_duration) as sized by
// relay/mod.rs:277-287.
#ifndef SRT_RELAY_COMMON_H
#define SRT_RELAY_COMMON_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SRT_HD __host__ __device__ __forceinline__
#else
#define SRT_HD inline
#endif

namespace relay {

constexpr uint64_t NONE = ~0ull;         // Option::None of the reference's EmulatedTime options
constexpr uint64_t MTU = 1500;           // CONFIG_MTU (definitions.h:124)
constexpr uint64_t REFILL_NS = 1000000;  // relay/mod.rs:278

SRT_HD uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
SRT_HD uint64_t sat_sub(uint64_t a, uint64_t b) { return a > b ? a - b : 0; }
SRT_HD uint64_t sat_mul(uint64_t a, uint64_t b) {
    uint64_t r;
    return __builtin_mul_overflow(a, b, &r) ? ~0ull : r;
}

SRT_HD void raise(uint32_t *flags, uint32_t bit) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(flags, bit);
#else
    *flags |= bit;
#endif
}

SRT_HD void add_pending(unsigned long long *total, unsigned long long n) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (n) atomicAdd(total, n);
#else
    *total += n;
#endif
}

SRT_HD uint32_t take_slot(uint32_t *count) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(count, 1u);
#else
    return (*count)++;
#endif
}

// ---- the walk of a batch grouped by host: ptr[0 .. n_hosts] are the hosts' bounds
// the packets the bounds cover, held inside the batch of n whatever ptr[] says
SRT_HD uint32_t walked(const uint32_t *ptr, uint32_t n_hosts, uint32_t n) {
    return ptr[n_hosts] < n ? ptr[n_hosts] : n;
}

// host h's segment, held below `lim` (walked) whatever ptr[] says
SRT_HD void segment(const uint32_t *ptr, uint32_t lim, uint32_t h, uint32_t &b, uint32_t &e) {
    b = ptr[h] < lim ? ptr[h] : lim;
    e = ptr[h + 1] < lim ? ptr[h + 1] : lim;
    if (e < b) e = b;
}

// records of a late list that exist: the count runs past the cap on overflow (nullptr: no late list)
SRT_HD uint32_t late_n(const uint32_t *count, uint32_t cap) {
    if (!count) return 0;
    const uint32_t n = *count;
    return n < cap ? n : cap;
}

// the scan's output for a host whose packets begin at `prefix`: positions stop at out_cap (a u32)
SRT_HD uint32_t host_base(uint64_t prefix, uint64_t out_cap) { return (uint32_t)(prefix < out_cap ? prefix : out_cap); }

// create_token_bucket's refill size (relay/mod.rs:277-287); the capacity is sat_add(refill, MTU)
SRT_HD uint64_t bucket_refill(uint64_t bytes_per_second) { return bytes_per_second / 1000 ? bytes_per_second / 1000 : 1; }

// TokenBucket::conforming_remove_inner (token_bucket.rs:75-157); false: *wait
SRT_HD bool bucket_remove(uint64_t &balance, uint64_t &last_refill, uint64_t refill, uint64_t capacity, uint64_t dec,
                          uint64_t now, uint64_t &wait) {
    uint64_t span = sat_sub(now, last_refill);
    if (span >= REFILL_NS) {  // lazy_refill
        const uint64_t n = span / REFILL_NS;
        const uint64_t b = sat_add(balance, sat_mul(refill, n));
        balance = b < capacity ? b : capacity;
        last_refill = sat_add(last_refill, sat_mul(REFILL_NS, n));
        span = sat_sub(now, last_refill);
    }
    const uint64_t next_refill = REFILL_NS - span;
    if (balance >= dec) {
        balance -= dec;
        return true;
    }
    const uint64_t need = dec - balance;
    const uint64_t refills = need / refill + (need % refill ? 1 : 0);
    wait = refills <= 1 ? next_refill : sat_add(next_refill, sat_mul(REFILL_NS, refills - 1));
    return false;
}

}  // namespace relay
#endif
