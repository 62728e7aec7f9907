"""Per-kernel comparison of two device assemblies of csrc/dhts_api.hip (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S, with the
build's -Xclang -target-feature -Xclang +unaligned-ds-access): every kernel's instructions and its .amdhsa_ resource block, with the
assembler's local labels left as they are.  usage: compare_device_asm.py parent.s change.s"""
import hashlib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", ln)
        if m and not m.group(1).startswith((".L", "BB")):
            if name:
                out[name] = body
            name, body = m.group(1), []
            if name.startswith("__hip_cuid_"):                 # the compilation unit's id, a hash of the source: not code
                name = None
        elif name is not None:
            s = ln.split(";")[0].rstrip()
            if s.strip() and "__hip_cuid_" not in s and not s.lstrip().startswith((".file", ".loc", ".ident", ".section", ".cfi")):
                body.append(s)
    if name:
        out[name] = body
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
print("symbols: parent %d, change %d; identical %d, different %d, only in parent %d, only in change %d"
      % (len(a), len(b), len(same), len(diff), len(set(a) - set(b)), len(set(b) - set(a))))
for k in sorted(diff) + sorted(set(a) ^ set(b)):
    print("DIFFERS" if k in diff else "ONE SIDE", k)
for k in sorted(same):
    print("%s %6d lines  %s" % (hashlib.sha256("\n".join(a[k]).encode()).hexdigest()[:16], len(a[k]), k))
