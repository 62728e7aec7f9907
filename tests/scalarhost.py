"""A DuckDB stand-in for the functions of register_kmer_udf_functions, in ctypes: the function-pointer table dhts_set_duckdb_api /
duckhts_init_c_api take, with the slots the family uses -- scalar and table functions, typed positional parameters, flat vectors,
duckdb_string_t in its inline and pointer forms, validity words, list and struct children.  It records what gets registered and calls a
registered function on a chunk built from Python lists.  (tests/minihost has no scalar functions and hands every positional parameter the
path.)  No compiler needed; slot numbers come from include/duckdb_abi_slots.h."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTOR_SIZE = 2048
TYPE_NAMES = {1: "BOOLEAN", 2: "TINYINT", 3: "SMALLINT", 4: "INTEGER", 5: "BIGINT", 6: "UTINYINT", 7: "USMALLINT", 8: "UINTEGER", 9: "UBIGINT", 10: "FLOAT", 11: "DOUBLE", 17: "VARCHAR"}
WIDTH = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 2, 8: 4, 9: 8, 10: 4, 11: 8, 17: 16}
CTYPE = {1: C.c_uint8, 2: C.c_int8, 3: C.c_int16, 4: C.c_int32, 5: C.c_int64, 6: C.c_uint8, 7: C.c_uint16, 8: C.c_uint32, 9: C.c_uint64, 10: C.c_float, 11: C.c_double}
_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]


class HostError(RuntimeError):
    pass


class LType:
    """a logical type: prim id, LIST(child) or STRUCT(names, children)"""
    def __init__(self, tid, child=None, fields=None):
        self.tid, self.child, self.fields = tid, child, fields

    def __str__(self):
        if self.tid == 24:
            return str(self.child) + "[]"
        if self.tid == 25:
            return "STRUCT(" + ", ".join(f"{n} {t}" for n, t in self.fields) + ")"
        return TYPE_NAMES[self.tid]


class Vec:
    """a flat vector of `cap` rows"""
    def __init__(self, t, cap=VECTOR_SIZE):
        self.t, self.cap = t, cap
        self.validity = None
        self.keep = []                                   # the string heap
        self.child, self.list_size, self.children = None, 0, []
        w = 16 if t.tid == 24 else 0 if t.tid == 25 else WIDTH[t.tid]
        self.buf = (C.c_uint8 * max(cap * w, 8))()
        if t.tid == 24:
            self.child = Vec(t.child, cap)
        if t.tid == 25:
            self.children = [Vec(ft, cap) for _, ft in t.fields]

    def ensure_validity(self):
        if self.validity is None:
            self.validity = (C.c_uint64 * ((self.cap + 63) // 64))(*([2 ** 64 - 1] * ((self.cap + 63) // 64)))

    def grow(self, cap):
        if cap <= self.cap:
            return
        new = Vec(self.t, max(cap, 2 * self.cap))
        C.memmove(new.buf, self.buf, len(self.buf))
        if self.validity is not None:
            new.ensure_validity()
            C.memmove(new.validity, self.validity, C.sizeof(self.validity))
        new.keep = self.keep
        self.__dict__.update(new.__dict__)

    def is_valid(self, i):
        return self.validity is None or bool(self.validity[i // 64] >> (i % 64) & 1)

    def set_invalid(self, i):
        self.ensure_validity()
        self.validity[i // 64] &= ~(1 << (i % 64)) & (2 ** 64 - 1)

    def put_string(self, i, b):
        rec = bytearray(16)
        rec[0:4] = len(b).to_bytes(4, "little")
        if len(b) <= 12:
            rec[4:4 + len(b)] = b
        else:
            heap = C.create_string_buffer(bytes(b), len(b))
            self.keep.append(heap)
            rec[4:8] = b[:4]
            rec[8:16] = C.addressof(heap).to_bytes(8, "little")
        C.memmove(C.addressof(self.buf) + 16 * i, bytes(rec), 16)

    def get_string(self, i):
        rec = bytes(self.buf[16 * i:16 * i + 16])
        n = int.from_bytes(rec[0:4], "little")
        return rec[4:4 + n] if n <= 12 else C.string_at(int.from_bytes(rec[8:16], "little"), n)

    def fill(self, values):
        """python values -> rows 0 .. len(values) - 1 (None = NULL; list children are appended behind list_size)"""
        for i, v in enumerate(values):
            if v is None:
                self.set_invalid(i)
                if self.t.tid == 24:
                    C.memmove(C.addressof(self.buf) + 16 * i, (self.list_size).to_bytes(8, "little") + bytes(8), 16)
                continue
            if self.t.tid == 17:
                self.put_string(i, v.encode() if isinstance(v, str) else bytes(v))
            elif self.t.tid == 24:
                self.child.grow(self.list_size + len(v))
                sub = Vec(self.t.child, max(len(v), 1)); sub.fill(v)
                w = WIDTH[self.t.child.tid]
                C.memmove(C.addressof(self.child.buf) + w * self.list_size, sub.buf, w * len(v))
                for k in range(len(v)):
                    if v[k] is None:
                        self.child.set_invalid(self.list_size + k)
                C.memmove(C.addressof(self.buf) + 16 * i, self.list_size.to_bytes(8, "little") + len(v).to_bytes(8, "little"), 16)
                self.list_size += len(v)
            else:
                C.cast(self.buf, C.POINTER(CTYPE[self.t.tid]))[i] = v
        return self

    def read(self, n):
        out = []
        if self.t.tid == 25:
            cols = [c.read(n) for c in self.children]
            return [[col[i] for col in cols] if self.is_valid(i) else None for i in range(n)]
        for i in range(n):
            if not self.is_valid(i):
                out.append(None)
            elif self.t.tid == 17:
                out.append(self.get_string(i))
            elif self.t.tid == 24:
                rec = bytes(self.buf[16 * i:16 * i + 16])
                o, ln = int.from_bytes(rec[:8], "little"), int.from_bytes(rec[8:], "little")
                p = C.cast(self.child.buf, C.POINTER(CTYPE[self.t.child.tid]))
                out.append([p[o + k] if self.child.is_valid(o + k) else None for k in range(ln)])
            else:
                v = C.cast(self.buf, C.POINTER(CTYPE[self.t.tid]))[i]
                out.append(bool(v) if self.t.tid == 1 else v)
        return out


class _Fn:
    def __init__(self, kind):
        self.kind, self.name, self.params, self.named, self.ret = kind, None, [], [], None
        self.extra = None
        self.cb = self.bind = self.init = self.func = None


class _Call:
    """the info object of one bind / init / function call"""
    def __init__(self, fn):
        self.fn, self.error = fn, None
        self.params, self.named = [], {}
        self.columns, self.cardinality = [], None
        self.bind_data = self.init_data = None
        self.max_threads = None


class Host:
    def __init__(self, lib):
        self.lib = lib
        self.objs, self.next_id = {}, 16
        self.registered = []                                 # _Fn in registration order
        self.unimplemented = []
        self.keep = []
        text = open(os.path.join(ROOT, "include", "duckdb_abi_slots.h")).read()
        self.slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SLOT_(duckdb_\w+) (\d+)", text)}
        n = int(re.search(r"#define DUCKDB_ABI_V120_NSLOTS (\d+)", text).group(1))
        self.table = (C.c_void_p * n)()
        self._build()

    # ---- handles ----
    def new(self, obj):
        self.next_id += 16
        self.objs[self.next_id] = obj
        return self.next_id

    def obj(self, h):
        return self.objs[h]

    def _set(self, name, restype, argtypes, fn):
        cb = C.CFUNCTYPE(restype, *argtypes)(fn)
        self.keep.append(cb)
        self.table[self.slots[name]] = C.cast(cb, C.c_void_p)

    def _build(self):
        P, U64, S, B = C.c_void_p, C.c_uint64, C.c_char_p, C.c_bool
        PP = C.POINTER(C.c_void_p)
        for name in self.slots:                              # a slot the family should not need records its name instead of crashing
            def trap(name=name):
                self.unimplemented.append(name)
                return 0
            self._set(name, P, [], trap)

        def drop(pp):
            if pp and pp[0]:
                self.objs.pop(pp[0], None)
                pp[0] = None
        self.table[self.slots["duckdb_malloc"]] = C.cast(_libc.malloc, C.c_void_p)
        self.table[self.slots["duckdb_free"]] = C.cast(_libc.free, C.c_void_p)
        self._set("duckdb_vector_size", U64, [], lambda: VECTOR_SIZE)

        def connect(db, out):
            out[0] = self.new("connection")
            return 0
        self._set("duckdb_connect", C.c_int, [P, PP], connect)
        self._set("duckdb_disconnect", None, [PP], drop)
        # logical types
        self._set("duckdb_create_logical_type", P, [C.c_int], lambda t: self.new(LType(t)))
        self._set("duckdb_create_list_type", P, [P], lambda c: self.new(LType(24, child=self.obj(c))))
        self._set("duckdb_create_map_type", P, [P, P], lambda k, v: self.new(LType(26)))
        self._set("duckdb_create_struct_type", P, [PP, C.POINTER(S), U64], lambda ts, ns, n: self.new(LType(25, fields=[(ns[i].decode(), self.obj(ts[i])) for i in range(n)])))
        self._set("duckdb_destroy_logical_type", None, [PP], drop)
        self._set("duckdb_get_type_id", C.c_int, [P], lambda t: self.obj(t).tid)
        self._set("duckdb_vector_get_column_type", P, [P], lambda v: self.new(self.obj(v).t))
        # scalar functions
        self._set("duckdb_create_scalar_function", P, [], lambda: self.new(_Fn("scalar")))
        self._set("duckdb_destroy_scalar_function", None, [PP], drop)
        self._set("duckdb_scalar_function_set_name", None, [P, S], lambda f, s: setattr(self.obj(f), "name", s.decode()))
        self._set("duckdb_scalar_function_add_parameter", None, [P, P], lambda f, t: self.obj(f).params.append(self.obj(t)))
        self._set("duckdb_scalar_function_set_return_type", None, [P, P], lambda f, t: setattr(self.obj(f), "ret", self.obj(t)))
        self._set("duckdb_scalar_function_set_extra_info", None, [P, P, P], lambda f, x, d: setattr(self.obj(f), "extra", x))
        self._set("duckdb_scalar_function_set_function", None, [P, P], lambda f, cb: setattr(self.obj(f), "cb", cb))

        def register(conn, f):
            self.registered.append(self.obj(f))
            return 0
        self._set("duckdb_register_scalar_function", C.c_int, [P, P], register)
        self._set("duckdb_scalar_function_get_extra_info", P, [P], lambda i: self.obj(i).fn.extra)
        self._set("duckdb_scalar_function_set_error", None, [P, S], lambda i, m: setattr(self.obj(i), "error", m.decode()))
        # table functions
        self._set("duckdb_create_table_function", P, [], lambda: self.new(_Fn("table")))
        self._set("duckdb_destroy_table_function", None, [PP], drop)
        self._set("duckdb_table_function_set_name", None, [P, S], lambda f, s: setattr(self.obj(f), "name", s.decode()))
        self._set("duckdb_table_function_add_parameter", None, [P, P], lambda f, t: self.obj(f).params.append(self.obj(t)))
        self._set("duckdb_table_function_add_named_parameter", None, [P, S, P], lambda f, s, t: self.obj(f).named.append((s.decode(), self.obj(t))))
        self._set("duckdb_table_function_set_bind", None, [P, P], lambda f, cb: setattr(self.obj(f), "bind", cb))
        self._set("duckdb_table_function_set_init", None, [P, P], lambda f, cb: setattr(self.obj(f), "init", cb))
        self._set("duckdb_table_function_set_local_init", None, [P, P], lambda f, cb: None)
        self._set("duckdb_table_function_set_function", None, [P, P], lambda f, cb: setattr(self.obj(f), "func", cb))
        self._set("duckdb_table_function_supports_projection_pushdown", None, [P, B], lambda f, b: None)
        self._set("duckdb_register_table_function", C.c_int, [P, P], register)
        # values and bind
        self._set("duckdb_bind_get_parameter", P, [P, U64], lambda i, k: self.new(("value", self.obj(i).params[k])) if k < len(self.obj(i).params) else None)
        self._set("duckdb_bind_get_parameter_count", U64, [P], lambda i: len(self.obj(i).params))
        self._set("duckdb_bind_get_named_parameter", P, [P, S], lambda i, s: self.new(("value", self.obj(i).named[s.decode()])) if s.decode() in self.obj(i).named else None)
        self._set("duckdb_is_null_value", B, [P], lambda v: self.obj(v)[1] is None)
        self._set("duckdb_get_int64", C.c_int64, [P], lambda v: int(self.obj(v)[1]))
        self._set("duckdb_get_bool", B, [P], lambda v: bool(self.obj(v)[1]))

        def get_varchar(v):
            s = self.obj(v)[1]
            s = s.encode() if isinstance(s, str) else bytes(s)
            p = _libc.malloc(len(s) + 1)
            C.memmove(p, s + b"\0", len(s) + 1)
            return p
        self._set("duckdb_get_varchar", P, [P], get_varchar)
        self._set("duckdb_destroy_value", None, [PP], drop)
        self._set("duckdb_bind_add_result_column", None, [P, S, P], lambda i, s, t: self.obj(i).columns.append((s.decode(), self.obj(t))))
        self._set("duckdb_bind_set_cardinality", None, [P, U64, B], lambda i, n, e: setattr(self.obj(i), "cardinality", (n, e)))
        self._set("duckdb_bind_set_bind_data", None, [P, P, P], lambda i, d, f: setattr(self.obj(i), "bind_data", (d, f)))
        self._set("duckdb_bind_set_error", None, [P, S], lambda i, m: setattr(self.obj(i), "error", m.decode()))
        self._set("duckdb_init_get_bind_data", P, [P], lambda i: self.obj(i).bind_data[0])
        self._set("duckdb_init_set_init_data", None, [P, P, P], lambda i, d, f: setattr(self.obj(i), "init_data", (d, f)))
        self._set("duckdb_init_set_max_threads", None, [P, U64], lambda i, n: setattr(self.obj(i), "max_threads", n))
        self._set("duckdb_init_set_error", None, [P, S], lambda i, m: setattr(self.obj(i), "error", m.decode()))
        self._set("duckdb_function_get_bind_data", P, [P], lambda i: self.obj(i).bind_data[0])
        self._set("duckdb_function_get_init_data", P, [P], lambda i: self.obj(i).init_data[0])
        self._set("duckdb_function_set_error", None, [P, S], lambda i, m: setattr(self.obj(i), "error", m.decode()))
        # chunks and vectors
        self._set("duckdb_data_chunk_get_vector", P, [P, U64], lambda c, k: self.obj(c)["handles"][k])
        self._set("duckdb_data_chunk_get_size", U64, [P], lambda c: self.obj(c)["size"])
        self._set("duckdb_data_chunk_set_size", None, [P, U64], lambda c, n: self.obj(c).__setitem__("size", n))
        self._set("duckdb_vector_get_data", P, [P], lambda v: C.addressof(self.obj(v).buf))
        self._set("duckdb_vector_get_validity", P, [P], lambda v: None if self.obj(v).validity is None else C.addressof(self.obj(v).validity))
        self._set("duckdb_vector_ensure_validity_writable", None, [P], lambda v: self.obj(v).ensure_validity())
        self._set("duckdb_validity_set_row_invalid", None, [C.POINTER(U64), U64], lambda w, r: w.__setitem__(r // 64, w[r // 64] & ~(1 << (r % 64)) & (2 ** 64 - 1)))
        self._set("duckdb_vector_assign_string_element_len", None, [P, U64, P, U64], lambda v, i, p, n: self.obj(v).put_string(i, C.string_at(p, n)))
        self._set("duckdb_vector_assign_string_element", None, [P, U64, S], lambda v, i, s: self.obj(v).put_string(i, s))
        self._set("duckdb_list_vector_get_child", P, [P], lambda v: self.handle_of(self.obj(v).child))
        self._set("duckdb_list_vector_get_size", U64, [P], lambda v: self.obj(v).list_size)

        def list_set_size(v, n):
            self.obj(v).list_size = n
            return 0

        def list_reserve(v, n):
            self.obj(v).child.grow(n)
            return 0
        self._set("duckdb_list_vector_set_size", C.c_int, [P, U64], list_set_size)
        self._set("duckdb_list_vector_reserve", C.c_int, [P, U64], list_reserve)
        self._set("duckdb_struct_vector_get_child", P, [P, U64], lambda v, k: self.handle_of(self.obj(v).children[k]))

    def handle_of(self, vec):
        if not hasattr(vec, "_h"):
            vec._h = self.new(vec)
        return vec._h

    # ---- the host's side ----
    def install(self):
        """dhts_set_duckdb_api: the library's callbacks read this table from now on"""
        self.lib.dhts_set_duckdb_api.argtypes = [C.c_void_p]
        self.lib.dhts_set_duckdb_api.restype = None
        self.lib.dhts_set_duckdb_api(C.addressof(self.table))

    def load_extension(self):
        """duckhts_init_c_api(info, access): what LOAD does"""
        GET_API = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p)
        GET_DB = C.CFUNCTYPE(C.c_void_p, C.c_void_p)
        SET_ERR = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

        class Access(C.Structure):
            _fields_ = [("set_error", SET_ERR), ("get_database", GET_DB), ("get_api", GET_API)]
        db = (C.c_void_p * 1)(0x10)
        errs = []
        acc = Access(SET_ERR(lambda i, m: errs.append(m)), GET_DB(lambda i: C.addressof(db)), GET_API(lambda i, v: C.addressof(self.table)))
        self.keep.append(acc)
        self.lib.duckhts_init_c_api.restype = C.c_bool
        self.lib.duckhts_init_c_api.argtypes = [C.c_void_p, C.c_void_p]
        ok = self.lib.duckhts_init_c_api(0x3, C.addressof(acc))
        if not ok or errs:
            raise HostError(f"duckhts_init_c_api failed: {errs}")

    def catalog(self):
        """[(name, [parameter types], return type or named parameters)] in registration order"""
        return [(f.name, [str(t) for t in f.params], str(f.ret) if f.kind == "scalar" else {n: str(t) for n, t in f.named}) for f in self.registered]

    def function(self, name):
        for f in self.registered:
            if f.name == name:
                return f
        raise KeyError(name)

    def call(self, name, *columns, output=None):
        """the scalar function on one chunk: columns are python lists of one length (<= VECTOR_SIZE); returns the output rows.
        output: an output vector to write into (one that already holds list children, say)"""
        self.install()
        f = self.function(name)
        n = len(columns[0])
        assert f.kind == "scalar" and len(columns) == len(f.params) and n <= VECTOR_SIZE
        vecs = [Vec(t).fill(col) for t, col in zip(f.params, columns)]
        out = output if output is not None else Vec(f.ret)
        chunk = self.new({"handles": [self.handle_of(v) for v in vecs], "size": n})
        info = _Call(f)
        hi = self.new(info)
        C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p)(f.cb)(hi, chunk, self.handle_of(out))
        if info.error is not None:
            raise HostError(info.error)
        self.last_output = out
        return out.read(n)

    def table_function(self, name, *params, **named):
        """bind, init and the scan of a table function: {"columns": [(name, type)], "cardinality": (n, exact), "rows": [tuple], "chunks": [sizes]}"""
        self.install()
        f = self.function(name)
        info = _Call(f)
        info.params, info.named = list(params), dict(named)
        hi = self.new(info)
        C.CFUNCTYPE(None, C.c_void_p)(f.bind)(hi)
        if info.error is not None:
            raise HostError(info.error)
        C.CFUNCTYPE(None, C.c_void_p)(f.init)(hi)
        if info.error is not None:
            raise HostError(info.error)
        rows, sizes = [], []
        try:
            while True:
                vecs = [Vec(t) for _, t in info.columns]
                chunk = {"handles": [self.handle_of(v) for v in vecs], "size": 0}
                C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)(f.func)(hi, self.new(chunk))
                if info.error is not None:
                    raise HostError(info.error)
                m = chunk["size"]
                if m == 0:
                    break
                sizes.append(m)
                rows += list(zip(*[v.read(m) for v in vecs]))
        finally:
            for data in (info.init_data, info.bind_data):
                if data and data[1]:
                    C.CFUNCTYPE(None, C.c_void_p)(data[1])(data[0])
        return {"columns": [(n, str(t)) for n, t in info.columns], "cardinality": info.cardinality, "max_threads": info.max_threads, "rows": rows, "chunks": sizes}


def load(env=None):
    """a Host over the built library, the extension loaded with `env` set (and the four opt-in variables cleared otherwise)"""
    import duckhts_amd
    for k in ("DHTS_KMER_FUNCTIONS", "DHTS_SEQ_FUNCTIONS", "DHTS_INTERVAL_FUNCTIONS", "DHTS_NUC_FUNCTIONS", "DHTS_TABIX_FUNCTIONS"):
        os.environ.pop(k, None)
    os.environ.update(env or {})
    try:
        h = Host(C.CDLL(duckhts_amd.LIB_PATH))
        h.load_extension()
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)
    return h
