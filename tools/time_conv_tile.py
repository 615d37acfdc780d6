"""Scratch (GPU box): time the 849-GFLOP 3x3x3 256->256 layer on one tile of the bf16x3 kernel through the C ABI.
   python tools/time_conv_tile.py [tile]   # an id of nerfdet_amd/conv_tiles.py (default 128)"""
import os, sys, ctypes, torch
from torch import nn
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerfdet_amd import conv3d as C3, _lib, conv_tiles
from ctypes import c_void_p
C3.set_arithmetic("bf16x3")
dev = torch.device("cuda")
conv = nn.Conv3d(256, 256, 3, 1, 1, bias=False).to(dev); bn = nn.BatchNorm3d(256).to(dev).eval()
pk = C3.packed([conv], bn)
x = torch.randn(60, 80, 50, 256, device=dev)
out = torch.empty(60, 80, 50, 256, device=dev)
planes = C3.split_planes(pk)
ws = torch.zeros(128, dtype=torch.int64, device=dev)
lib = _lib.load()
st = c_void_p(torch.cuda.current_stream().cuda_stream)
TILE = int(sys.argv[1]) if len(sys.argv) > 1 else 128
assert TILE in conv_tiles.TILES, f"tile: one of {conv_tiles.SPLIT_IDS}"
args = _lib.NdetConvArgs(size=ctypes.sizeof(_lib.NdetConvArgs), in_=x.data_ptr(), w_planes=planes.data_ptr(), out=out.data_ptr(), D=60, H=80, W=50,
                         Cin=256, Cout=256, kernel=(3, 3, 3), stride=(1, 1, 1), pad=(1, 1, 1), scale=pk.scale.data_ptr(), shift=pk.shift.data_ptr(),
                         relu=1, splits=1, tile=TILE, arith=0, workspace=ws.data_ptr())
ts = []
for i in range(6):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = lib.ndet_conv_split(args, st)
    e1.record(); torch.cuda.synchronize(); assert rc == 0
    ts.append(e0.elapsed_time(e1))
print("TILE", TILE, "ms", sorted(ts)[2], "TF", 2*240000*256*6912/sorted(ts)[2]/1e9, flush=True)

