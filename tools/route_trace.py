"""Which conv kernels a bench-shaped step launches, as a multiset that two builds can be compared on.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/route_trace.py run
    python tools/route_trace.py reduce DIR > profiles/route_trace_NAME.txt

run: ONE bf16 training step (forward, loss, backward) of the bench network: 8 bands, base 64, bilinear, B = 16, 256 x 256.
reduce: the newest kernel trace under DIR as sorted lines `count kernel grid(workgroups) workgroup_size lds_bytes`, conv and
weight-gradient kernels only (lds = the trace's LDS_Block_Size, which counts a kernel's static LDS only: the dynamic LDS of the
conv kernels is a compile-time constant of each instantiation).  tests/test_conv_route_cpu.py's bench table was checked against these lines."""
import collections
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    import torch
    from floodplanet_code_amd import _lib
    from floodplanet_code_amd.unet import HipUNet
    from tools.step_digest import train_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = HipUNet(8, 2, base_channels=64, precision="bf16").to(dev).train()
    x, tgt = torch.rand(16, 8, 256, 256, device=dev), torch.randint(0, 2, (16, 256, 256), device=dev)
    print(train_step(_lib.load(), net, x, tgt))


def reduce(d):
    f = max(glob.glob(d + "/**/*kernel_trace.csv", recursive=True), key=os.path.getmtime)
    n = collections.Counter()
    for r in csv.DictReader(open(f)):
        name = re.sub(r"^void ", "", r["Kernel_Name"]).split("(")[0].replace("fu::", "")
        if not (name.startswith("k_conv3x3") or name.startswith("k_wgrad")):
            continue
        wg = int(r["Workgroup_Size_X"])
        n[(name, int(r["Grid_Size_X"]) // wg, wg, r.get("LDS_Block_Size", "?"))] += 1
    for (name, grid, wg, lds), c in sorted(n.items()):
        print(f"{c:3d} {name} grid={grid} wg={wg} lds={lds}")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else reduce(sys.argv[2])
