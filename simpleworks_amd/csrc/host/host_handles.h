// Host-only handles of the C ABI (include/swmarlin.h): a generator and a verifying key.
#pragma once
#include <new>
#include "ahp.h"

struct swm_rng {
    swm::ChaChaRng r;
};
struct swm_vk {
    swm::VerifyingKey vk;
};

// Body of an extern "C" entry point: MarlinError -> its code, bad_alloc -> SWM_ERR_OOM, anything else -> SWM_ERR_INTERNAL.
// Needs swm::set_err and swm::drain_streams declared at the point of use.
#define SWM_GUARD(ctx, body)                                  \
    try {                                                     \
        body;                                                 \
        return SWM_OK;                                        \
    } catch (const MarlinError& e) {                          \
        drain_streams(ctx);                                   \
        set_err(ctx, e.code, "%s", e.what());                 \
        return e.code;                                        \
    } catch (const std::bad_alloc&) {                         \
        drain_streams(ctx);                                   \
        return SWM_ERR_OOM;                                   \
    } catch (const std::exception& e) {                       \
        drain_streams(ctx);                                   \
        set_err(ctx, SWM_ERR_INTERNAL, "%s", e.what());       \
        return SWM_ERR_INTERNAL;                              \
    }
