"""Command line of the package: ``python -m tamp_amd compress|decompress|index|append|read|build-dictionary`` with the options of the reference's CLI.

Mirrors ``tamp/cli/main.py:115-232`` (``tamp compress`` / ``tamp decompress``: ``--input/-i``, ``--output/-o``,
``--window/-w``, ``--literal/-l``, ``--dictionary/-d``, ``--lazy-matching``, ``--extended`` / ``--no-extended``; stdin /
stdout when no path is given; "No data provided." on empty input) and its dictionary rule (``main.py:90-105``): a
dictionary file of exactly ``1 << window`` bytes is used as it is, a shorter one is raw effective bytes -- the seeded
default fills the buffer and the file's contents are copied to its END -- a longer one is an error.  The codec work
runs on the GPU through the same ``tamp_amd.compress`` / ``tamp_amd.decompress`` as everything else; there is no
``--implementation`` choice to make.  ``build-dictionary`` (``tamp/cli/build_dictionary.py:706-927``: a custom dictionary
from a corpus of messages) is ``tamp_amd/build_dictionary.py``: same options and output contract, every whole-corpus
evaluation one batch launch on the GPU.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from typing import Optional


def load_dictionary(path, window: int, literal: int, extended: bool) -> bytearray:
    """The reference CLI's dictionary rule (tamp/cli/main.py:90-105): a file of exactly the window size IS the window; a
    shorter one is placed at the END of a seeded window (v1 streams seed with the literal-8 alphabet); a longer one is
    refused."""
    import tamp_amd

    payload = Path(path).read_bytes()
    capacity = 1 << window
    if len(payload) > capacity:
        raise ValueError(f"Dictionary file ({len(payload)} bytes) is larger than window size ({capacity} bytes).")
    if len(payload) == capacity:
        return bytearray(payload)
    seeded = tamp_amd.initialize_dictionary(capacity, literal=literal if extended else 8)
    seeded[capacity - len(payload):] = payload
    return seeded


def _slurp(path: Optional[str]) -> bytes:
    """Whole input from a file, or from stdin when no path was given; empty input is an error like in the reference."""
    blob = Path(path).read_bytes() if path is not None else sys.stdin.buffer.read()
    if len(blob) == 0:
        raise ValueError("No data provided.")
    return blob


def _deliver(path: Optional[str], blob: bytes) -> None:
    if path is not None:
        Path(path).write_bytes(blob)
        return
    sys.stdout.buffer.write(blob)


def _bits(lo: int, hi: int):
    def parse(text: str) -> int:
        v = int(text)
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError(f"must be in [{lo}, {hi}]")
        return v

    return parse


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="tamp_amd", description="Compress/Decompress data in Tamp format (on an MI355X).")
    sub = ap.add_subparsers(dest="command", required=True)
    for name, help_ in (("compress", "Compress an input file or stream."), ("decompress", "Decompress an input file or stream.")):
        p = sub.add_parser(name, help=help_)
        p.add_argument("input_pos", nargs="?", default=None, metavar="INPUT", help="input file (default: stdin)")
        p.add_argument("output_pos", nargs="?", default=None, metavar="OUTPUT", help="output file (default: stdout)")
        p.add_argument("--input", "-i", default=None)
        p.add_argument("--output", "-o", default=None)
        p.add_argument("--window", "-w", type=_bits(8, 15), default=10, help="bits of the dictionary window")
        p.add_argument("--literal", "-l", type=_bits(5, 8), default=8, help="bits of a literal")
        p.add_argument("--dictionary", "-d", default=None, help="custom initialization dictionary (binary file)")
        p.add_argument("--extended", action=argparse.BooleanOptionalAction, default=True)
        if name == "compress":
            p.add_argument("--lazy-matching", action=argparse.BooleanOptionalAction, default=False)
            p.add_argument("--reset-interval", type=int, default=None, metavar="N",
                           help="reset the dictionary every N input bytes (sets the header's dictionary_reset bit): the "
                                "segments between resets are compressed in parallel, at some cost in ratio")
    x = sub.add_parser("index", help="Find the dictionary resets of compressed files: entries, interval, decoded size.")
    x.add_argument("files", nargs="+", metavar="FILE")
    a = sub.add_parser("append", help="Append a file's bytes to a stream compressed with --reset-interval; its segments stay N bytes long.")
    a.add_argument("stream", metavar="STREAM", help="the compressed file")
    a.add_argument("input", metavar="INPUT", help="the bytes to append")
    a.add_argument("--output", "-o", default=None, help="the new stream (default: STREAM is rewritten, through a temporary file and a rename)")
    a.add_argument("--reset-interval", type=int, default=None, metavar="N",
                   help="the interval the stream was compressed with (needed only while it has no closed segment to tell it by)")
    a.add_argument("--lazy-matching", action=argparse.BooleanOptionalAction, default=False)
    r = sub.add_parser("read", help="Read a byte range of a compressed file with dictionary resets, decoding only the segments it touches.")
    r.add_argument("file", metavar="FILE", help="the compressed file; its segments may be of any size")
    r.add_argument("--begin", "-b", type=_bits(0, (1 << 64) - 1), required=True, metavar="B", help="the range's first decoded byte")
    r.add_argument("--length", "-n", type=_bits(0, 0xFFFFFFFF), required=True, metavar="L", help="decoded bytes to read")
    r.add_argument("--output", "-o", default=None, help="output file (default: stdout)")
    b = sub.add_parser("build-dictionary", help="Build a custom dictionary from a corpus of messages.")
    b.add_argument("input", metavar="INPUT", help="directory of sample files, or one file cut at --delimiter")
    b.add_argument("--output", "-o", default="dictionary.bin", help="binary dictionary file (effective bytes only)")
    b.add_argument("--window", "-w", type=_bits(8, 15), default=10)
    b.add_argument("--literal", "-l", type=_bits(5, 8), default=8)
    b.add_argument("--extended", action=argparse.BooleanOptionalAction, default=True)
    b.add_argument("--delimiter", default="\n", help="splits a single input file into samples (default: newline)")
    b.add_argument("--trim-threshold", "-t", type=_bits(2, 1 << 15), default=None,
                   help="shortest substring worth an entry (default: a few values are tried, the best one kept)")
    b.add_argument("--target-fill", "-f", type=float, default=None, help="fraction of the window to fill (default: the knee)")
    b.add_argument("--quiet", "-q", action="store_true")
    return ap


def _append(tamp_amd, args) -> int:
    """``append STREAM INPUT``: the index comes from ``index_resets``, the interval from it or from ``--reset-interval``."""
    import os

    try:
        blob, more = Path(args.stream).read_bytes(), Path(args.input).read_bytes()
        scan = tamp_amd.index_resets([blob])
        if int(scan.status[0]) not in (0, 2):
            raise ValueError(f"{args.stream}: not a stream whose resets can be found (status {int(scan.status[0])})")
        interval = scan.index.interval if int(scan.index.first[1]) else None
        if interval is None:
            interval = args.reset_interval
        elif args.reset_interval is not None and args.reset_interval != interval:
            raise ValueError(f"{args.stream}: its segments hold {interval} bytes, not {args.reset_interval}")
        if interval is None:
            raise ValueError(f"{args.stream}: no closed segment of a regular size yet: pass --reset-interval")
        res = tamp_amd.append_batch([blob], reset_index=scan.index, reset_interval=interval, source=[more], lazy_matching=args.lazy_matching)
        if int(res.status[0]) != 0:
            raise ValueError(f"{args.stream}: the append failed with status {int(res.status[0])}")
        if args.output is not None:
            Path(args.output).write_bytes(res.stream(0))
            return 0
        tmp = args.stream + ".tmp%d" % os.getpid()
        try:
            Path(tmp).write_bytes(res.stream(0))
            os.replace(tmp, args.stream)
        except OSError:
            if os.path.exists(tmp):
                os.unlink(tmp)  # (nothing is left next to STREAM)
            raise
    except (OSError, ValueError) as e:
        print(f"tamp_amd: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
    return 0


def _read(tamp_amd, args) -> int:
    """``read FILE --begin B --length L``: the index comes from ``index_resets``, the grid from its table of segment ends."""
    try:
        blob = Path(args.file).read_bytes()
        if len(blob) < 1 or not blob[0] & 1:
            raise ValueError(f"{args.file}: the stream has no dictionary resets (its header's reset bit is not set): decompress it instead")
        scan = tamp_amd.index_resets([blob])
        if int(scan.status[0]) != 0:
            raise ValueError(f"{args.file}: not a stream whose resets can be found (status {int(scan.status[0])})")
        res = tamp_amd.read_ranges([blob], reset_index=scan.index, segment_ends=scan.segment_ends(), stream_index=[0],
                                   begin=[args.begin], length=[args.length])
        if int(res.status[0]) not in (0, 2):
            raise ValueError(f"{args.file}: the read failed with status {int(res.status[0])}")
    except (OSError, ValueError) as e:
        print(f"tamp_amd: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
    _deliver(args.output, res.range(0))
    return 0


def main(argv=None) -> int:
    import tamp_amd

    args = build_parser().parse_args(argv)
    if args.command == "build-dictionary":
        from tamp_amd import build_dictionary as bd

        if args.target_fill is not None and not 0.0 < args.target_fill <= 1.0:
            print("tamp_amd: --target-fill must be in (0, 1]", file=sys.stderr)
            return 2
        try:
            bd.build_dictionary_cli(args.input, args.output, window=args.window, literal=args.literal, extended=args.extended,
                                    delimiter=args.delimiter, trim_threshold=args.trim_threshold,
                                    target_fill=args.target_fill, quiet=args.quiet)
        except ValueError as e:
            print(f"tamp_amd: {type(e).__name__}: {e}", file=sys.stderr)
            return 1
        return 0
    if args.command == "index":
        scan = tamp_amd.index_resets([Path(f).read_bytes() for f in args.files])
        from tamp_amd.batch import _detect_interval

        for i, f in enumerate(args.files):  # (the interval of each file's own segments; scan.index.interval is the batch's)
            a, b = int(scan.index.first[i]), int(scan.index.first[i + 1])
            own = _detect_interval(scan.index.first[i:i + 2] - scan.index.first[i], scan.closed_size[a:b], scan.open_size[i:i + 1],
                                   scan.status[i:i + 1])
            print(f"{f}: status {int(scan.status[i])}, {b - a} resets, interval {own or 'none'}, {scan.size(i)} bytes decoded")
        return 0
    if args.command == "append":
        return _append(tamp_amd, args)
    if args.command == "read":
        return _read(tamp_amd, args)
    src = args.input if args.input is not None else args.input_pos
    dst = args.output if args.output is not None else args.output_pos
    try:
        data = _slurp(src)
        kwargs = {}
        if args.dictionary is not None:
            kwargs["dictionary"] = load_dictionary(args.dictionary, args.window, args.literal, args.extended)
        if args.command == "compress":
            if args.reset_interval is not None:
                kwargs.update(dictionary_reset=True, reset_interval=args.reset_interval)
            out = tamp_amd.compress(data, window=args.window, literal=args.literal, lazy_matching=args.lazy_matching,
                                    extended=args.extended, **kwargs)
        else:
            out = tamp_amd.decompress(data, **kwargs)
    except (ValueError, IndexError, tamp_amd.ExcessBitsError) as e:
        print(f"tamp_amd: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
    _deliver(dst, bytes(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
