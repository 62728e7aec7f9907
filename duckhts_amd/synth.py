"""Deterministic synthetic BGZF BAM inputs -- workload tooling.

Thin ctypes wrapper over tools/synth_bam.c (system libz.so.1, level-6 raw deflate, 65280-byte
payloads cut without regard to record boundaries) and tools/synth_gpu.hip (the same bytes made on
the device: the records by the shared model, the deflate by a restatement of zlib level 6).
Not part of the scan path.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "tools", "libsynth.so")
_GPU_SO = os.path.join(_ROOT, "tools", "libsynth_gpu.so")
_DEPS = [os.path.join(_ROOT, "tools", f) for f in ("synth_bam_model.h", "zlib6_deflate.h")]
_LIB = None
_GPU_LIB = None


def _stale(target, srcs):
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(s) for s in srcs)


def build(force=False, gpu=True):
    src = os.path.join(_ROOT, "tools", "synth_bam.c")
    if force or _stale(_SO, [src] + _DEPS):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-pthread", "-o", _SO, src,
                               "-l:libz.so.1"])
    gsrc = os.path.join(_ROOT, "tools", "synth_gpu.hip")
    if gpu and (force or _stale(_GPU_SO, [gsrc] + _DEPS)):
        hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", _GPU_SO, gsrc,
                               "-l:libz.so.1"])
    return _SO


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            build()
        L = C.CDLL(_SO)
        L.synth_bam_segment.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        L.synth_bam_segment.restype = C.c_size_t
        L.synth_bcf_segment.argtypes = L.synth_bam_segment.argtypes
        L.synth_bcf_segment.restype = C.c_size_t
        L.synth_zlib6_block.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.synth_zlib6_block.restype = C.c_size_t
        _LIB = L
    return _LIB


def _gpu_lib():
    global _GPU_LIB
    if _GPU_LIB is None:
        if not os.path.exists(_GPU_SO):
            build()
        L = C.CDLL(_GPU_SO)
        L.synth_gpu_bam_segments.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int,
                                             C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.synth_gpu_bam_segments.restype = C.c_int64
        L.synth_gpu_error.restype = C.c_char_p
        _GPU_LIB = L
    return _GPU_LIB


def zlib6_block(raw) -> bytes:
    """raw deflate of one BGZF payload (<= 65,280 bytes) by the restatement of zlib level 6 the device runs, on the host;
    b"" where zlib would not fit the stream in a BGZF block (bgzf_block then stores it)"""
    src = np.frombuffer(bytes(raw), np.uint8)
    dst = np.empty(65536, np.uint8)
    n = _lib().synth_zlib6_block(src.ctypes.data, src.nbytes, dst.ctypes.data)
    if n == C.c_size_t(-1).value:
        raise ValueError("zlib6_block: at most 65,280 bytes")
    return dst[:n].tobytes()


def bam_segments_gpu(n, k0, nseg, seed=42, total_n=None, device=0, group=2, out=None):
    """Segments k0 .. k0+nseg-1 of n records each (records [k*n, (k+1)*n) of a total_n-record file), made on the device: the bytes of
    bam_segment(n, seed, total_n, rec0=k*n, with_header=False, with_eof=False) for every k, concatenated -> (uint8 array, per-segment byte
    sizes, inflated bytes).  `group` segments share one device pass (about 25 GB of device memory per segment of 4 M records)."""
    total_n = n * (k0 + nseg) if total_n is None else total_n
    cap = int(n) * nseg * 260 + (1 << 20)
    if out is None:
        out = np.empty(cap, dtype=np.uint8)
    sizes = (C.c_uint64 * nseg)()
    raw = C.c_uint64(0)
    L = _gpu_lib()
    got = L.synth_gpu_bam_segments(device, seed, total_n, n, k0, nseg, group, out.ctypes.data, out.nbytes, sizes, C.byref(raw))
    if got < 0:
        raise RuntimeError("synth_gpu_bam_segments: " + L.synth_gpu_error().decode())
    return out[:got], [int(x) for x in sizes], int(raw.value)


def bam_segment(n, seed=42, total_n=None, rec0=0, with_header=True, with_eof=True, level=6, payload=65280,
                threads=None, out=None):
    """Records [rec0, rec0+n) of a conceptual total_n-record file -> (uint8 array, stats dict).

    `out` may be a preallocated uint8 numpy array (e.g. pinned memory); otherwise one is allocated.
    """
    total_n = n if total_n is None else total_n
    threads = threads or min(os.cpu_count() or 1, 32)
    cap = int(n) * 260 + (1 << 20)
    if out is None:
        out = np.empty(cap, dtype=np.uint8)
    stats = (C.c_uint64 * 2)()
    got = _lib().synth_bam_segment(seed, total_n, rec0, n, int(with_header), int(with_eof), level, payload, threads,
                                   out.ctypes.data, out.nbytes, stats)
    if got == 0:
        raise RuntimeError("synth_bam_segment: output capacity too small")
    return out[:got], {"raw_bytes": int(stats[0]), "n_blocks": int(stats[1]), "n_records": int(n)}


def bam_file(n, seed=42, **kw) -> bytes:
    arr, _ = bam_segment(n, seed=seed, **kw)
    return arr.tobytes()


def bcf_segment(n, seed=43, total_n=None, rec0=0, with_header=True, with_eof=True, level=6, payload=65280, threads=None, out=None):
    """Synthetic 16-sample BCF records [rec0, rec0+n) -> (uint8 array, stats dict)."""
    total_n = n if total_n is None else total_n
    threads = threads or min(os.cpu_count() or 1, 32)
    cap = int(n) * 700 + (1 << 20)
    if out is None:
        out = np.empty(cap, dtype=np.uint8)
    stats = (C.c_uint64 * 2)()
    got = _lib().synth_bcf_segment(seed, total_n, rec0, n, int(with_header), int(with_eof), level, payload, threads, out.ctypes.data, out.nbytes, stats)
    if got == 0:
        raise RuntimeError("synth_bcf_segment: output capacity too small")
    return out[:got], {"raw_bytes": int(stats[0]), "n_blocks": int(stats[1]), "n_records": int(n)}


def bcf_file(n, seed=43, **kw) -> bytes:
    arr, _ = bcf_segment(n, seed=seed, **kw)
    return arr.tobytes()
