// hip_event_pair.h -- the two events of a timed span, destroyed on every exit path (rx_host.h: timed_loop; ring.hip)
#pragma once
#include <hip/hip_runtime.h>

struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
