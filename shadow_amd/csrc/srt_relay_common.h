// srt_relay_common.h -- what the inbound and the outbound relay steps share
// (srt_inbound_step.h, srt_outbound_step.h): the saturating u64 arithmetic of
// the reference's SimulationTime / token counts, the host-or-device updates of
// the call-wide words, and the relay's TokenBucket.
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
