"""Compressor(lazy_matching=True) as a bounded-memory writer: N bytes of the prose corpus (tiled) in 1 MiB writes, then close().
Prints wall time, the bytes that had left when the last write returned, and the largest len(_pending) seen -- the bytes the object
held in host memory.  TAMP_AMD_TREE names another checkout to import tamp_amd from (for a measurement of an earlier commit).
usage: python tools/lazy_write_bench.py [bytes = 100000000] [lazy = 1]   (GPU box)"""
import json, os, sys, time
sys.path.insert(0, os.environ.get('TAMP_AMD_TREE') or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tamp_amd
from tamp_amd import workloads as wl

total = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
lazy = bool(int(sys.argv[2])) if len(sys.argv) > 2 else True
prose = wl.real_text('prose')
step = 1 << 20


class Count:
    n = 0
    def write(self, b): self.n += len(b)
    def flush(self): pass


tamp_amd.compress(prose[:70_000], lazy_matching=lazy)  # (library load, context, kernel code object: not what is measured)
sink = Count()
c = tamp_amd.Compressor(sink, lazy_matching=lazy)
held = at = 0
t0 = time.perf_counter()
while at < total:
    k = min(step, total - at)
    o = at % len(prose)
    chunk = prose[o:o + k]
    while len(chunk) < k:
        chunk += prose[:k - len(chunk)]
    c.write(chunk)
    held = max(held, len(c._pending))
    at += k
t_write, out_write = time.perf_counter() - t0, sink.n
c.close()
t_all = time.perf_counter() - t0
print(json.dumps(dict(tree=os.environ.get('TAMP_AMD_TREE_LABEL', 'this checkout'), lazy_matching=lazy, input_bytes=total,
                      write_bytes=step, output_bytes=sink.n, output_bytes_when_last_write_returned=out_write,
                      seconds_in_writes=round(t_write, 3), seconds_total=round(t_all, 3), mb_per_s=round(total / t_all / 1e6, 2),
                      largest_pending_bytes=held, piece_max=tamp_amd.Compressor.PIECE_MAX)), flush=True)
