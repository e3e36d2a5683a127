"""Times the MJPEG decoder on 1280x720 4:2:2 streams and writes profiles/mjpeg_time.txt or profiles/mjpeg_split_time.txt.

    python tests/golden/make_mjpeg_golden.py --timing 32 gpu_jobs/mjpeg_720p     # needs Pillow; the folder is not committed
    python tools/time_mjpeg.py --streams gpu_jobs/mjpeg_720p [--out profiles/mjpeg_time.txt] [--only N RST [SPLIT]]
    python tools/time_mjpeg.py --streams gpu_jobs/mjpeg_720p --root OTHER_CHECKOUT --baseline base.json
    python tools/time_mjpeg.py --streams gpu_jobs/mjpeg_720p --split [--parent base.json] [--out profiles/mjpeg_split_time.txt]

Host streams -> device RGB (rtdm_mjpeg_decode_batch_device + a stream synchronisation), ms per frame at 1, 16 and 256 frames per
call, with restart intervals of one MCU row (rst_*.jpg) and without (norst_*.jpg); the files are cycled to fill a call.  Where
Pillow imports, its single-thread Image.open(...).load() over the same streams is the library baseline; otherwise the file says
that it was not measured.  --only N RST [SPLIT] runs that one case a few times and writes nothing (for a kernel trace).

--split times the frames without restart intervals only: 1, 2, 16 and 256 frames per call with one lane per segment (split = 0) and
with subsequences of 64 .. 1024 bytes (rtdm_mjpeg_set_split), and notes the most rounds a frame took with each row.  --baseline
FILE times 1 and 2 frames per call three times over with whatever build --root names (a checkout of the parent commit, built) and
stores the figures; --parent FILE puts them into the table: their spread is what a difference has to exceed to count."""
import argparse
import glob
import importlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = (64, 128, 256, 512, 1024)


def load(folder, tag):
    files = sorted(glob.glob(os.path.join(folder, tag + "_*.jpg")))
    if not files:
        raise SystemExit("no %s_*.jpg in %s" % (tag, folder))
    return [open(f, "rb").read() for f in files]


def time_case(pkg, torch, frames, n, reps, split=None, stats=None):
    """best ms per frame of `reps` calls of n frames; split: rtdm_mjpeg_set_split's value (None: the build's default); stats: a
    list that gets the handle's split_stats() appended"""
    dec = pkg.HIPMJPEGDecoder(1280, 720, max_batch=n, max_stream_bytes=max(len(f) for f in frames))
    if split is not None:
        dec.split = split
    batch = [frames[i % len(frames)] for i in range(n)]
    out = torch.empty((n, 720, 1280, 3), dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    for _ in range(2):
        dec.decode_batch(batch, out=out, status=status)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        dec.decode_batch(batch, out=out, status=status)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    if stats is not None:
        stats.append(dec.split_stats())
    dec.close()
    return best * 1e3 / n


def pillow_lines(sets):
    lines = []
    try:
        from PIL import Image
        for tag in sets:
            t0 = time.perf_counter()
            for s in sets[tag]:
                Image.open(io.BytesIO(s)).load()
            lines.append("Pillow %s single thread, Image.open(...).load(), %s: %.3f ms per frame"
                         % (Image.__version__, tag, (time.perf_counter() - t0) * 1e3 / len(sets[tag])))
    except ImportError:
        lines.append("Pillow single thread: not measured (Pillow does not import on this machine)")
    return lines


def baseline(pkg, torch, frames, path):
    """1 and 2 frames per call, three times over, with the build that was imported -> path (JSON)"""
    out = {str(n): [time_case(pkg, torch, frames, n, 8) for _ in range(3)] for n in (1, 2)}
    json.dump(out, open(path, "w"))
    print(out)


def split_table(pkg, torch, frames, parent, out):
    counts = (1, 2, 16, 256)
    lines = ["MJPEG decoder, frames WITHOUT restart intervals (one entropy segment each): 1280x720 4:2:2 quality 85 as Pillow writes",
             "them, host streams -> device RGB (rtdm_mjpeg_decode_batch_device + stream sync), best of the repetitions, ms per frame;",
             "%d distinct streams, cycled; mean stream %.0f KB.  device: %s" % (len(frames), sum(map(len, frames)) / len(frames) / 1e3,
                                                                             torch.cuda.get_device_name(0)),
             "split: bytes per subsequence (rtdm_mjpeg_set_split); 0 = one lane per segment.  In brackets: the most rounds of",
             "speculative decoding a frame of the row took / the subsequences per frame (mean).  A frame is cut into 1024 at the",
             "most, so settings below len / 1024 give one and the same cut.", "",
             "%-22s" % "frames per call" + "".join("%22d" % n for n in counts)]
    table, cut = {}, {}
    for split in (0,) + SPLITS:
        cells = []
        for n in counts:
            stats = []
            ms = time_case(pkg, torch, frames, n, 8 if n < 256 else 4, split, stats)
            table[(split, n)] = ms
            cut[split] = round(stats[0][1] / max(1, stats[0][0]))
            cells.append("%12.3f [%2d /%5d]" % (ms, stats[0][2], cut[split]))
        lines.append("%-22s" % ("split = %d" % split) + "".join(cells))
    lines.append("")
    if parent:
        base = json.load(open(parent))
        for n in (1, 2):
            v = base[str(n)]
            lines.append("parent commit's build, %d per call, three times over: %s   spread %.3f ms"
                         % (n, "  ".join("%.3f" % x for x in v), max(v) - min(v)))
        again = {n: [time_case(pkg, torch, frames, n, 8, 0) for _ in range(3)] for n in (1, 2)}
        for n in (1, 2):
            lines.append("this build at split = 0, %d per call, three times over: %s" % (n, "  ".join("%.3f" % x for x in again[n])))
        lines.append("")
    best2 = min(SPLITS, key=lambda s: table[(s, 2)])
    lines.append("fastest at 2 frames per call (left + right, the reference's call): split = %d; the same cut: split = %s"
                 % (best2, ", ".join(str(s) for s in SPLITS if cut[s] == cut[best2])))
    lines += [""] + pillow_lines({"norst": frames})
    text = "\n".join(lines) + "\n"
    print(text)
    open(out, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", required=True)
    ap.add_argument("--out")
    ap.add_argument("--only", nargs="+", metavar="N RST [SPLIT]")
    ap.add_argument("--root", default=ROOT, help="the checkout whose build is timed")
    ap.add_argument("--baseline", metavar="FILE")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--parent", metavar="FILE")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    pkg = importlib.import_module("rt-depth-map_amd")
    sets = {"rst": load(a.streams, "rst"), "norst": load(a.streams, "norst")}
    if a.only:
        n, tag, split = int(a.only[0]), a.only[1], (int(a.only[2]) if len(a.only) > 2 else None)
        print("%s n=%d: %.3f ms per frame" % (tag, n, time_case(pkg, torch, sets[tag], n, 3, split)))
        return
    if a.baseline:
        return baseline(pkg, torch, sets["norst"], a.baseline)
    if a.split:
        return split_table(pkg, torch, sets["norst"], a.parent, a.out or os.path.join(ROOT, "profiles", "mjpeg_split_time.txt"))
    a.out = a.out or os.path.join(ROOT, "profiles", "mjpeg_time.txt")
    lines = ["MJPEG decoder, 1280x720 4:2:2 quality 85, host streams -> device RGB (rtdm_mjpeg_decode_batch_device + stream sync)",
             "best of the repetitions, ms per frame; %d distinct streams per kind, cycled; mean stream %.0f / %.0f KB (rst / norst)"
             % (len(sets["rst"]), sum(map(len, sets["rst"])) / len(sets["rst"]) / 1e3,
                sum(map(len, sets["norst"])) / len(sets["norst"]) / 1e3),
             "device: %s" % torch.cuda.get_device_name(0), "",
             "%-28s %10s %10s %10s" % ("frames per call", 1, 16, 256)]
    for tag, label in (("rst", "restart every MCU row"), ("norst", "no restart intervals")):
        info = pkg.mjpeg_probe(sets[tag][0])
        ms = [time_case(pkg, torch, sets[tag], n, 8 if n < 256 else 4) for n in (1, 16, 256)]
        lines.append("%-28s %10.3f %10.3f %10.3f   (%d segments per frame)" % (label, ms[0], ms[1], ms[2], info["segments"]))
    lines.append("")
    lines += pillow_lines(sets)
    text = "\n".join(lines) + "\n"
    print(text)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
