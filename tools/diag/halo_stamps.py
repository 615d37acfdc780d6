"""GPU box: shader-clock stamps of tile 3128 (k_conv_split_halo<4,2>) in the fp16-pair arithmetic, one tap per barrier interval (the switch of
ndet_conv_halo_taps forced to 1) against three.  Needs a library whose conv_split_kernels.hip was compiled with -DHALO_STAMPS=1 (stamps around the
barriers only) or -DHALO_STAMPS=2 (also an s_waitcnt lgkmcnt(0) + stamp between the fragment reads and the first MFMA of an interval: splits reads
from MFMAs, and serialises them), linked with the other objects as the Makefile does, in place of nerf-det_amd/lib/libnerfdet_hip.so.
Every wave of workgroup (0, 0, 0) sums the ticks of each part of its K walk; printed per barrier interval and per tap.
profiles/r05_a_halo3128_kstep_stamps.txt holds what this produced."""
import ctypes, os, sys
import torch
from torch import nn
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from nerfdet_amd import _lib, conv3d as C
lib = _lib.load()
raw = ctypes.CDLL(_lib.LIB_PATH)
raw.ndet_halo_set_stamps.argtypes = [ctypes.c_void_p]
dev = torch.device("cuda")
torch.manual_seed(0)
C.set_arithmetic("f16x2")
LAYERS = [("l3.conv2 3x3 256->256 50x15x20", 2, (50, 15, 20), 256, 256, 9), ("neck out0 3x3x3 256->128 40x40x16", 3, (40, 40, 16), 256, 128, 27)]
buf = torch.zeros(8 * 4, dtype=torch.int64, device=dev)
for name, dim, grid, cin, cout, taps in LAYERS:
    conv = (nn.Conv2d if dim == 2 else nn.Conv3d)(cin, cout, 3, 1, 1, bias=False).to(dev)
    bn = (nn.BatchNorm2d if dim == 2 else nn.BatchNorm3d)(cout).to(dev).eval()
    pk = C.packed([conv], bn)
    x = torch.relu(torch.randn(*grid, cin, device=dev))
    run = (lambda: C.conv2d_nhwc(x, pk, relu=1, tile=3128, splits=1)) if dim == 2 else (lambda: C.conv3d_ndhwc(x, pk, relu=1, tile=3128, splits=1))
    steps = taps * cin // 32
    for mode in (1, 0):
        _lib.check(lib.ndet_conv_halo_taps(mode, 0, 0, 0, None, None), "conv_halo_taps")
        with torch.no_grad():
            for _ in range(3):
                run()
            ts = []
            for _ in range(9):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); run(); e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            buf.zero_()
            assert raw.ndet_halo_set_stamps(ctypes.c_void_p(buf.data_ptr())) == 0
            run()
            torch.cuda.synchronize()
            raw.ndet_halo_set_stamps(ctypes.c_void_p(0))
        s = buf.view(8, 4).cpu().double()
        tps = 1 if mode == 1 else 3
        iv = steps // tps
        print(f"{name} tile 3128 f16x2, {tps} tap(s) per interval: {steps} taps, {iv} intervals; launch {sorted(ts)[4]:.1f} us (p10 {sorted(ts)[1]:.1f}, p90 {sorted(ts)[7]:.1f}; stamped build)")
        for w in range(8):
            role = "consumer" if w < 4 else "producer"
            parts = ("reads", "MFMAs (+reads at level 1)", "P1", "P2") if w < 4 else ("DMA issue+wait", "P1", "restage", "P2+next image loads")
            tot = float(s[w].sum())
            print(f"  wave {w} {role}: " + " | ".join(f"{p} {float(s[w, i]) / iv:7.0f}" for i, p in enumerate(parts)) + f" | per interval {tot / iv:7.0f} | per tap {tot / steps:7.0f}")
_lib.check(lib.ndet_conv_halo_taps(0, 0, 0, 0, None, None), "conv_halo_taps")
