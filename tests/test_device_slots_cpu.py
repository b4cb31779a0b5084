"""DeviceSlots (csrc/fu_device_slots.h), the per-device once-only bookkeeping behind the CU count and the dynamic-LDS
opt-in of the conv launchers: 8 host threads ask for 4 device indices many times with a counting fill function.  Each
index is filled exactly once, every thread reads the filled value, and an index outside the capacity calls its fill
function every time and never sees another index's value.  A stand-alone program with its own main, built with
-fsanitize=thread where the host compiler has that runtime (plain otherwise) and run directly.  Needs no GPU and no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "floodplanet_code_amd", "csrc")

PROGRAM = r"""
#include "fu_device_slots.h"
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

static fu::DeviceSlots slots;
static std::atomic<int> fills[4];
static std::atomic<int> ready{0};
static std::atomic<long> far_fills{0};
static std::atomic<int> bad{0};

static void worker(int t) {
  ready.fetch_add(1);
  while (ready.load() < 8) std::this_thread::yield();          // all threads reach the first get() together
  for (int it = 0; it < 20000; ++it) {
    const int dev = (it + t) & 3;
    const int v = slots.get(dev, [dev] { fills[dev].fetch_add(1); return 1000 + dev; });
    if (v != 1000 + dev) bad.fetch_add(1);
    if (it % 100 == 0) {                                        // at and beyond the capacity, and below zero: never remembered
      const int outside[3] = {fu::DeviceSlots::CAP, fu::DeviceSlots::CAP + 3 + t, -1 - t};
      for (int far : outside) {
        const int w = slots.get(far, [far] { far_fills.fetch_add(1); return 7000 + far; });
        if (w != 7000 + far) bad.fetch_add(1);
      }
    }
  }
}

int main() {
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t) th.emplace_back(worker, t);
  for (auto& x : th) x.join();
  std::printf("fills %d %d %d %d far %ld bad %d\n", fills[0].load(), fills[1].load(), fills[2].load(), fills[3].load(),
              far_fills.load(), bad.load());
  return 0;
}
"""

TRIVIAL = "int main() { return 0; }\n"


def host_compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def build(cxx, src, out, extra):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-I", CSRC, *extra, str(src), "-o", str(out)],
                          capture_output=True, text=True)


def test_device_slots_fill_once_from_eight_threads(tmp_path):
    cxx = host_compiler()
    assert cxx, "no host C++ compiler found"
    (tmp_path / "trivial.cpp").write_text(TRIVIAL)
    (tmp_path / "slots.cpp").write_text(PROGRAM)
    # the ThreadSanitizer runtime is used where an empty program builds and runs with it
    tsan = ["-fsanitize=thread"]
    probe = build(cxx, tmp_path / "trivial.cpp", tmp_path / "trivial", tsan)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "trivial")], capture_output=True).returncode != 0:
        tsan = []
    print("ThreadSanitizer:", "on" if tsan else "not available, plain build")
    b = build(cxx, tmp_path / "slots.cpp", tmp_path / "slots", tsan)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r =subprocess.run([str(tmp_path / "slots")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr, r.stderr
    # 8 threads x 200 rounds x 3 indices outside the capacity: every one of those calls ran its own fill
    assert r.stdout.strip() == "fills 1 1 1 1 far 4800 bad 0", r.stdout
