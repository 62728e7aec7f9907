"""occupancy.py KERNEL CODE_OBJECT [CODE_OBJECT ...] -- resident workgroups per CU of one kernel (block of 64, no dynamic LDS) as the HIP
runtime computes them, for each code object: hipModuleOccupancyMaxActiveBlocksPerMultiprocessor.  A code object is dhts_api.hip compiled
with the build's flags plus `--cuda-device-only --no-gpu-bundle-output` (A/B runs: one of the parent, one of the change)."""
import ctypes as C
import sys


def main():
    hip = C.CDLL("libamdhip64.so")
    kernel = sys.argv[1].encode()

    def ck(r, what):
        if r != 0:
            raise SystemExit(f"{what}: hip error {r}")

    ck(hip.hipInit(0), "hipInit")
    ck(hip.hipSetDevice(0), "hipSetDevice")
    for path in sys.argv[2:]:
        mod, fn, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        ck(hip.hipModuleLoad(C.byref(mod), path.encode()), "hipModuleLoad " + path)
        ck(hip.hipModuleGetFunction(C.byref(fn), mod, kernel), "hipModuleGetFunction")
        ck(hip.hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(C.byref(n), fn, 64, C.c_size_t(0)), "occupancy query")
        print(f"{path}: {sys.argv[1]} block=64: {n.value} workgroups per CU", flush=True)
        ck(hip.hipModuleUnload(mod), "hipModuleUnload")


if __name__ == "__main__":
    main()
