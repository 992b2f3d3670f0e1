// scratch_owner.hpp -- hand-over of thread-local scratch between the streams of one host thread.
// The handle-free entry points (reorder.hip, ellipsoid.hip, mixed.hip, hertz_friction.hip) keep grow-only device buffers
// per host thread, and return without synchronising: the same thread calling again on ANOTHER stream would use the
// histogram / keys / counters / board while the first stream's kernels still do.  Each such scratch carries an owner
// record, and every entry point that touches the scratch claims it before its first use (its reserve() included: a
// growing buffer is freed).  Entry points whose scratch is only ever used by calls that synchronise before they return
// (growth.hip, halo.hip, the blocking reductions of convex.hip) need none.
// The scratch is made of mhip_internal.hpp's DeviceBuffer, which has no destructor (thread_local objects would call
// hipFree during teardown); what a heap-allocated handle owns is a HandleBuffer, defined next to it.
#pragma once
#include "mhip_internal.hpp"

namespace mhip {

struct ScratchOwner {
  hipStream_t last = nullptr;  // the stream of the previous claim (nullptr is the null stream: `used` tells)
  bool used = false;
  hipEvent_t handover = nullptr;  // created at the first change of stream
  // Same stream as last time: one compare, nothing recorded.  Another stream: an event recorded NOW on the previous
  // stream lies behind its last use of the scratch (everything the thread has enqueued there so far); the new stream
  // waits for it.  The previous stream must still exist; if it does not (the record is refused), its work has been
  // drained by its destruction or is drained here by a device synchronisation.
  // Like the scratch itself (DeviceBuffer has no destructor: thread_local objects would call into HIP during teardown)
  // the event is never destroyed: one event per scratch per thread that ever changed streams.  Nor is the record aware
  // of devices, any more than the scratch is: a thread that changes the current device between two calls gets the
  // fallback, which drains the device current NOW -- use the handle-free entry points of a thread on one device.
  int claim(hipStream_t s) {
    if (used && s == last) return MHIP_SUCCESS;
    if (used) {
      if (!handover) MHIP_HIP(hipEventCreateWithFlags(&handover, hipEventDisableTiming));
      if (hipEventRecord(handover, last) == hipSuccess) {
        MHIP_HIP(hipStreamWaitEvent(s, handover, 0));
      } else {
        (void)hipGetLastError();
        MHIP_HIP(hipDeviceSynchronize());
      }
    }
    last = s;
    used = true;
    return MHIP_SUCCESS;
  }
};

}  // namespace mhip
