"""Times the MJPEG decoder on 1280x720 4:2:2 streams and writes profiles/mjpeg_time.txt.

    python tests/golden/make_mjpeg_golden.py --timing 32 gpu_jobs/mjpeg_720p     # needs Pillow; the folder is not committed
    python tools/time_mjpeg.py --streams gpu_jobs/mjpeg_720p [--out profiles/mjpeg_time.txt] [--only N RST]

Host streams -> device RGB (rtdm_mjpeg_decode_batch_device + a stream synchronisation), ms per frame at 1, 16 and 256 frames per
call, with restart intervals of one MCU row (rst_*.jpg) and without (norst_*.jpg); the files are cycled to fill a call.  Where
Pillow imports, its single-thread Image.open(...).load() over the same streams is the library baseline; otherwise the file says
that it was not measured.  --only N RST runs that one case a few times and writes nothing (for a kernel trace)."""
import argparse
import glob
import importlib
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(folder, tag):
    files = sorted(glob.glob(os.path.join(folder, tag + "_*.jpg")))
    if not files:
        raise SystemExit("no %s_*.jpg in %s" % (tag, folder))
    return [open(f, "rb").read() for f in files]


def time_case(pkg, torch, frames, n, reps):
    dec = pkg.HIPMJPEGDecoder(1280, 720, max_batch=n, max_stream_bytes=max(len(f) for f in frames))
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
    dec.close()
    return best * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpeg_time.txt"))
    ap.add_argument("--only", nargs=2, metavar=("N", "RST"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("rt-depth-map_amd")
    sets = {"rst": load(a.streams, "rst"), "norst": load(a.streams, "norst")}
    if a.only:
        n, tag = int(a.only[0]), a.only[1]
        print("%s n=%d: %.3f ms per frame" % (tag, n, time_case(pkg, torch, sets[tag], n, 3)))
        return
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
    try:
        from PIL import Image
        for tag in ("rst", "norst"):
            t0 = time.perf_counter()
            for s in sets[tag]:
                Image.open(io.BytesIO(s)).load()
            lines.append("Pillow %s single thread, Image.open(...).load(), %s: %.3f ms per frame"
                         % (Image.__version__, tag, (time.perf_counter() - t0) * 1e3 / len(sets[tag])))
    except ImportError:
        lines.append("Pillow single thread: not measured (Pillow does not import on this machine)")
    text = "\n".join(lines) + "\n"
    print(text)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
