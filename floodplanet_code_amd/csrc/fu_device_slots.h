// One int per device index, made on first use: the host-only bookkeeping behind the per-device launch facts of
// fu_common.h (CU count, dynamic-LDS opt-in of a kernel).  Nothing of HIP in here, so it builds and is tested alone
// (tests/test_device_slots_cpu.py).
#pragma once
#include <mutex>

namespace fu {

struct DeviceSlots {
  static constexpr int CAP = 32;   // device indices that are remembered; an index outside [0, CAP) calls fill() every time
  std::once_flag once[CAP];
  int val[CAP] = {};
  // fill() runs exactly once per index, whichever threads ask; every caller gets its value.  After that a call is
  // call_once's check of a set flag and one load: no lock, nothing asked of the runtime.
  template <typename F> int get(int dev, F&& fill) {
    if (dev < 0 || dev >= CAP) return fill();
    std::call_once(once[dev], [&] { val[dev] = fill(); });
    return val[dev];
  }
};

}  // namespace fu
