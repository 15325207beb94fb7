"""Vector instructions of k_gather per phase (the method of tools/encoder_valu_budget.py: one launch per stop stamp under a counter pass).
Needs the trace build (`make -C gpujpeg_amd/csrc trace`). Run under the counter pass, a run of its own:

    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d <dir> -- python tools/gather_valu_budget.py --run [--pattern camera]
    python tools/gather_valu_budget.py --report <dir>

--run encodes bench.py's 8K frame once per stop stamp (every wave of k_gather ends at stamp n: gj_hip_trace_stop_gather) and once in full, in that
order; --report reads the counter CSV, takes the k_gather dispatches in order and prints the differences per wave."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAMPS = ["set-up: tile, place in the file, result words, scan header", "segment books", "rounds"]
# what the work needs per wave of one ordinary 8K tile stream (~300 dwords, 7 segments), written down before measuring:
#   set-up: 4 group-total loads with their bounds ~ 16, the tile sizes in front ~ 5, two wave sums of 6 + a readlane, the byte counts and the first
#           rounds' loads ~ 12, the result words and the header copy in a few waves only -> ~ 50
#   books:  one wave prefix sum of the segments' dwords, the note of a segment's end ~ 20
#   rounds: per 256 dwords: 4 x 4 for the 0xFF masks, 4 counts, ~ 8 for the lane's output bytes, 6 + 3 for the prefix sum and the carry, ~ 6 for
#           the test and the store -> ~ 45; a lane with a segment's end or a 0xFF byte places its dwords one by one ~ 40, and the few dwords
#           with either go byte by byte ~ 40 a turn, one or two turns a round -> ~ 150 a round, two rounds
IDEAL = [50, 20, 300]
IDEAL_END = 2

ap = argparse.ArgumentParser()
ap.add_argument("--run", action="store_true")
ap.add_argument("--report", default=None)
ap.add_argument("--workload", default="8k")
ap.add_argument("--pattern", default="natural")
args = ap.parse_args()

if args.run:
    import ctypes as C
    import torch
    import bench
    from gpujpeg_amd import libgpujpeg as G
    lib = G.Library(os.environ.get("GJ_TRACE_LIB") or os.path.join(ROOT, "gpujpeg_amd", "lib", "libgpujpeg_trace.so"))
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    dev = torch.device("cuda", 0)
    spec = bench.Spec(lib, args.workload, args.pattern, 75, dev, 12345)
    L = bench.Lanes(lib, spec, dev, 1)
    L.set_stats(False)
    ln = L.lanes[0]
    lib.L.gj_hip_trace_stop_gather.argtypes = [C.c_int]
    for stop in list(range(1, len(STAMPS) + 1)) + [1 << 30]:
        assert lib.L.gj_hip_trace_stop_gather(stop) == 0
        try:
            L.encode(ln)
        except Exception:
            pass  # (a stopped launch leaves no valid stream: the call may report that)
        torch.cuda.synchronize()
    print("launched", len(STAMPS) + 1, "encodes")
    sys.exit(0)

rows = []
for f in glob.glob(os.path.join(args.report, "**", "*counter_collection.csv"), recursive=True):
    rows += list(csv.DictReader(open(f)))
gat = {}
for r in rows:
    if "k_gather" not in r["Kernel_Name"]:
        continue
    d = gat.setdefault(int(r["Dispatch_Id"]), {})
    d[r["Counter_Name"]] = float(r["Counter_Value"])
ids = sorted(gat)[-(len(STAMPS) + 1):]
vals = [gat[i]["SQ_INSTS_VALU"] for i in ids]
waves = gat[ids[-1]]["SQ_WAVES"]
print(f"k_gather, {args.workload}: {int(waves)} waves, SQ_INSTS_VALU of the complete kernel {vals[-1] / 1e6:.3f} M = {vals[-1] / waves:.1f} per wave")
print(f"{'phase':64s} {'measured / wave':>16s} {'ideal':>8s}")
prev = 0.0
for name, v, ideal in zip(STAMPS, vals, IDEAL):
    print(f"{name:64s} {(v - prev) / waves:16.1f} {ideal:8d}")
    prev = v
print(f"{'end (behind the last stamp)':64s} {(vals[-1] - prev) / waves:16.1f} {IDEAL_END:8d}")
print(f"{'sum':64s} {vals[-1] / waves:16.1f} {sum(IDEAL) + IDEAL_END:8d}")
