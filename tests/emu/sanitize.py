"""The emulations of tests/emu/*_host.py as STAND-ALONE programs under the host sanitizers.  A host module's text (_PRE + section() + _POST) gets a `main` of its own and
is compiled with the sanitizer's runtime linked statically, so nothing of it is ever loaded into python and nothing depends on the load order of the environment:
    asan   -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all      a read or write past the end of an array, by one byte
    tsan   -fsanitize=thread                                                               a lane's LDS access that no barrier orders against another lane's
The arguments of one call travel in one flat binary file, the arrays after the call in another.  The `main` reads every array into an allocation of its own of EXACTLY
the array's bytes (never rounded up, never carved out of a shared block), so that the redzone begins at the byte behind what include/a1mpc.h states for the argument; a
null pointer stays null; two arguments that are the same numpy array are the same allocation (the in-place cases).

    lib = sanitize.Library(plant_host, "asan")          # builds once per source text (write-then-rename under the temp directory, as the host modules do)
    lib.plant_run(n, stride, ..., state, None, ...)      # numpy arrays, None, numbers, or what the host modules' run() pass to ctypes
    with sanitize.instead_of_load(plant_host, lib): plant_host.run(...)     # the host module's own marshalling, on the sanitized program

A non-zero exit status raises SanitizerReport with the first report of the run."""
import contextlib, ctypes as C, hashlib, os, re, subprocess, tempfile, time
import numpy as np

FLAGS = dict(asan=["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
             tsan=["-fsanitize=thread", "-static-libtsan"])
COMMON = ["-O1", "-g1", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wno-unknown-pragmas"]
RUN_LIMIT_S = 120

# ---- the flat file: int64 words (entry, n_int, n_dbl, n_arr, n_fix), the integers, the doubles, n_arr x (bytes or -1 for null, alias or -1), n_fix x (table, word, target,
# offset), then the bytes of every array that is neither null nor an alias.  Back: (return value, n_arr), the bytes of those arrays in the same order.
_IO = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
namespace sanio {
struct Arr { unsigned char* p; int64_t bytes, alias; };
static int64_t entry, n_int, n_dbl, n_arr, n_fix;
static int64_t* ints; static double* dbls; static Arr* arr;
static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "sanio: %s\n", what); std::exit(3); } }
static void get(std::FILE* f, void* to, size_t bytes) { need(bytes == 0 || std::fread(to, 1, bytes, f) == bytes, "short input file"); }
static void load(const char* path) {
    std::FILE* f = std::fopen(path, "rb"); need(f != nullptr, "no input file");
    int64_t head[5]; get(f, head, sizeof head);
    entry = head[0]; n_int = head[1]; n_dbl = head[2]; n_arr = head[3]; n_fix = head[4];
    ints = new int64_t[n_int]; dbls = new double[n_dbl]; arr = new Arr[n_arr];
    get(f, ints, 8 * n_int); get(f, dbls, 8 * n_dbl);
    for (int64_t k = 0; k < n_arr; ++k) { int64_t w[2]; get(f, w, sizeof w); arr[k] = Arr{nullptr, w[0], w[1]}; }
    int64_t* fix = new int64_t[4 * n_fix]; get(f, fix, 32 * n_fix);
    for (int64_t k = 0; k < n_arr; ++k)
        if (arr[k].bytes >= 0 && arr[k].alias < 0) { arr[k].p = new unsigned char[arr[k].bytes]; get(f, arr[k].p, arr[k].bytes); }   // its own, exact-fit
    for (int64_t k = 0; k < n_arr; ++k)
        if (arr[k].alias >= 0) arr[k].p = arr[arr[k].alias].p;
    for (int64_t k = 0; k < n_fix; ++k) {   // a word of a table of addresses <- the address of an allocation of this process
        const int64_t* x = fix + 4 * k;
        const int64_t at = reinterpret_cast<int64_t>(arr[x[2]].p + x[3]);
        std::memcpy(arr[x[0]].p + 8 * x[1], &at, 8);
    }
    delete[] fix; std::fclose(f);
}
static void save(const char* path, int64_t ret) {
    std::FILE* f = std::fopen(path, "wb"); need(f != nullptr, "no output file");
    const int64_t head[2] = {ret, n_arr};
    std::fwrite(head, 1, sizeof head, f);
    for (int64_t k = 0; k < n_arr; ++k)
        if (arr[k].bytes >= 0 && arr[k].alias < 0) { std::fwrite(arr[k].p, 1, arr[k].bytes, f); delete[] arr[k].p; }
    delete[] ints; delete[] dbls; delete[] arr;
    need(std::fclose(f) == 0, "output file not written");
}
}
'''


class SanitizerReport(AssertionError):
    pass


def entries(post):
    """the extern "C" functions of a host module's _POST -> {name: (returns a value, [(C type, is a pointer)])}"""
    out = {}
    for ret, name, params in re.findall(r'extern "C"\s+([\w ]+?)\s+(\w+)\(([^)]*)\)\s*\{', post):
        ps = []
        for p in (q.strip() for q in params.split(",") if q.strip()):
            ty = p[:re.search(r"\w+$", p).start()].strip()
            ps.append((ty, "*" in ty))
        out[name] = (ret.strip() != "void", ps)
    return out


def call_main(post):
    """the `main` fragment for a host module: argv[1] is the call, argv[2] the arrays after it; one `case` per extern "C" function of _POST, its scalars in the order of
    the file's integers / doubles, its pointers in the order of the file's arrays"""
    cases = []
    for e, (name, (has_ret, ps)) in enumerate(entries(post).items()):
        i = d = a = 0; args = []
        for ty, ptr in ps:
            if ptr:
                args.append(f"reinterpret_cast<{ty.replace('const ', '')}>(sanio::arr[{a}].p)"); a += 1
            elif ty in ("double", "float"):
                args.append(f"static_cast<{ty}>(sanio::dbls[{d}])"); d += 1
            else:
                args.append(f"static_cast<{ty}>(sanio::ints[{i}])"); i += 1
        call = f"{name}({', '.join(args)})"
        cases.append(f"    case {e}: sanio::need(sanio::n_int == {i} && sanio::n_dbl == {d} && sanio::n_arr >= {a}, \"{name}: argument counts\"); "
                     + (f"ret = static_cast<int64_t>({call});" if has_ret else f"{call};") + " break;")
    return _IO + "int main(int argc, char** argv) {\n    sanio::need(argc == 3, \"usage: program call-file result-file\");\n    sanio::load(argv[1]);\n    int64_t ret = 0;\n" \
        "    switch (sanio::entry) {\n" + "\n".join(cases) + "\n    default: sanio::need(false, \"no such entry\");\n    }\n    sanio::save(argv[2], ret);\n    return 0;\n}\n"


def build(source, sanitizer, name, extra_flags=(), stats=None):
    """source text -> the path of the program, compiled once per (text, flags): <temp>/a1mpc_sanitize_<uid>/<name>_<sanitizer>_<hash> (a directory per user: one that
    another user made cannot be written to)"""
    flags = COMMON + FLAGS[sanitizer] + list(extra_flags)
    tag = hashlib.sha256((source + " ".join(flags)).encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), f"a1mpc_sanitize_{os.getuid()}"); os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, f"{name}_{sanitizer}_{tag}")
    if not os.path.exists(exe):
        cpp = exe + ".cpp"   # (the name carries the text's hash: whoever else writes it writes the same bytes)
        fd, part = tempfile.mkstemp(dir=d, prefix=os.path.basename(cpp) + ".")   # a name of this call's own: threads and processes may build side by side
        with os.fdopen(fd, "w") as f:
            f.write(source)
        os.replace(part, cpp)
        fd, tmp = tempfile.mkstemp(dir=d, prefix=os.path.basename(exe) + ".")
        os.close(fd)
        t0 = time.time()
        r = subprocess.run(["g++"] + flags + [cpp, "-o", tmp], capture_output=True, text=True)
        if r.returncode != 0:
            os.unlink(tmp)
        assert r.returncode == 0, f"{name} under {sanitizer} does not compile:\n{r.stderr[-4000:]}"
        os.chmod(tmp, 0o755)
        os.replace(tmp, exe)
        if stats is not None:
            stats["build_s"] = time.time() - t0
    return exe


def first_report(stderr, lines=30):
    rows = stderr.splitlines()
    for k, row in enumerate(rows):
        if re.search(r"ERROR: \w+Sanitizer|WARNING: ThreadSanitizer|runtime error:", row):
            return "\n".join(rows[k:k + lines])
    return "\n".join(rows[-lines:])


def run(exe, call_file, result_file, limit_s=RUN_LIMIT_S):
    """-> (exit status, stderr, result_file); the environment is passed on as it is"""
    r = subprocess.run([exe, call_file, result_file], capture_output=True, text=True, timeout=limit_s)
    return r.returncode, r.stderr, result_file


def _array_of(v):
    if v is None or isinstance(v, np.ndarray):
        return v
    if isinstance(v, C.c_void_p):   # numpy's ndarray.ctypes.data_as keeps the array on the pointer it returns
        if v.value is None:
            return None
        a = getattr(v, "_arr", None)
        assert isinstance(a, np.ndarray) and a.ctypes.data == v.value, "a pointer argument must come from ndarray.ctypes.data_as, so that its size is known"
        return a
    raise TypeError(f"pointer argument of type {type(v)}")


class Library:
    """what a host module's load() returns, but every call is one run of the sanitized stand-alone program.  `body`: the text between _PRE and _POST where the module
    compiles more than its own section(); `pre`: the module's preamble where it borrows another module's"""
    def __init__(self, module, sanitizer, body=None, pre=None, main=None, extra_flags=()):
        self.name, self.sanitizer = module.__name__.split(".")[-1], sanitizer
        self.pre = pre if pre is not None else module._PRE
        self.body = body if body is not None else module.section()
        self.post = module._POST
        self.main = main if main is not None else call_main(self.post)
        self.entries = entries(self.post)
        self.extra_flags = tuple(extra_flags)
        self.stats = {}
        self._exe = None

    def source(self):
        return self.pre + self.body + self.post + self.main

    def exe(self):
        if self._exe is None:
            self._exe = build(self.source(), self.sanitizer, self.name, self.extra_flags, stats=self.stats)
        return self._exe

    def __getattr__(self, name):
        if name.startswith("_") or name not in self.entries:
            raise AttributeError(name)
        return lambda *args, **kw: self.call(name, *args, **kw)

    def call(self, name, *args, fixups=(), extra=()):
        """fixups: [(table array, word, target array, byte offset)]: that int64 word of the table becomes the address of the target's allocation in the program, plus the
        offset; `extra`: further arrays that are no argument but a fix-up's target.  The arrays come back changed in place."""
        has_ret, ps = self.entries[name]
        assert len(args) == len(ps), f"{name} takes {len(ps)} arguments"
        ints, dbls, arrs = [], [], []
        for v, (ty, ptr) in zip(args, ps):
            v = v if ptr else getattr(v, "value", v)
            if ptr:
                arrs.append(_array_of(v))
            elif ty in ("double", "float"):
                dbls.append(float(v))
            else:
                ints.append(int(v) & 0xFFFFFFFFFFFFFFFF)
        arrs += list(extra)
        for a in arrs:
            assert a is None or a.flags.c_contiguous
        table, owned = [], []
        for k, a in enumerate(arrs):
            if a is None:
                table.append((-1, -1)); continue
            same = [j for j in owned if arrs[j].ctypes.data == a.ctypes.data and arrs[j].nbytes == a.nbytes]
            lo, hi = a.ctypes.data, a.ctypes.data + a.nbytes
            assert same or not any(arrs[j].ctypes.data < hi and lo < arrs[j].ctypes.data + arrs[j].nbytes for j in owned), "arguments overlap in part"
            if same:
                table.append((a.nbytes, same[0]))
            else:
                table.append((a.nbytes, -1)); owned.append(k)
        idx = lambda t: next(k for k, a in enumerate(arrs) if a is t)
        fix = [(idx(t), w, idx(g), off) for t, w, g, off in fixups]
        head = np.array([list(self.entries).index(name), len(ints), len(dbls), len(arrs), len(fix)], dtype=np.int64)
        blob = [head.tobytes(), np.array(ints, dtype=np.uint64).tobytes(), np.array(dbls, dtype=np.float64).tobytes(), np.array(table, dtype=np.int64).tobytes(),
                np.array(fix, dtype=np.int64).tobytes()] + [arrs[k].tobytes() for k in owned]
        exe = self.exe()
        with tempfile.TemporaryDirectory(prefix="a1mpc_sanitize_run_") as d:
            cf, rf = os.path.join(d, "call.bin"), os.path.join(d, "result.bin")
            with open(cf, "wb") as f:
                f.write(b"".join(blob))
            t0 = time.time()
            status, err, _ = run(exe, cf, rf)
            self.stats["run_s"] = max(self.stats.get("run_s", 0.0), time.time() - t0)
            if status != 0:
                raise SanitizerReport(f"{self.name}.{name} under {self.sanitizer}: exit status {status}\n{first_report(err)}")
            got = open(rf, "rb").read()
        ret, n_arr = np.frombuffer(got[:16], dtype=np.int64)
        assert n_arr == len(arrs) and len(got) == 16 + sum(arrs[k].nbytes for k in owned)
        at = 16
        for k in owned:
            a = arrs[k]
            if a.flags.writeable:
                a.reshape(-1).view(np.uint8)[:] = np.frombuffer(got[at:at + a.nbytes], dtype=np.uint8)
            at += a.nbytes
        return int(ret) if has_ret else None


@contextlib.contextmanager
def instead_of_load(module, lib):
    """inside, the host module's load() is `lib`: its own run() marshals for the sanitized program"""
    keep = module.load
    module.load = lambda: lib
    try:
        yield lib
    finally:
        module.load = keep


# ---- the solver source (csrc/a1mpc_solver.hpp on the host fibers of emu_harness.cpp) under asan: one program per horizon (-DA1_EMU_ONLY_H), because the harness as one
# sanitized unit does not fit a compiler.  ThreadSanitizer has nothing to see here: the fibers share one thread.
_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "a1-qp-mpc-controller_amd", "csrc")
SOLVER_SOURCES = ("emu_harness.cpp", "a1mpc_rowops.hpp")
SOLVER_HEADERS = ("a1mpc_solver.hpp", "a1mpc_tables.hpp")
# one process is one call, so the harness's three switches travel with it
SOLVER_POST = r'''
static void san_modes(int twin, int contact_stride, double* carry) { a1mpc_emu_set_twin(twin); a1mpc_emu_set_contact_stride(contact_stride); a1mpc_emu_set_carry(carry); }
extern "C" int san_solve(int twin, int contact_stride, double* carry, const a1mpc::DeviceParams* P, int horizon, int n, const double* x0, const double* xref, const double* R,
                         const double* foot, const uint8_t* contact, double* grf, double* u_full, double* warm_x, double* warm_y, double* rho, int32_t* iters,
                         int32_t* status, int32_t* nfact) {
    san_modes(twin, contact_stride, carry);
    return a1mpc_emu_solve(P, horizon, n, x0, xref, R, foot, contact, grf, u_full, warm_x, warm_y, rho, iters, status, nfact);
}
extern "C" int san_solve_split(int twin, int contact_stride, double* carry, const a1mpc::DeviceParams* P, int horizon, int n, int nrows, const double* x0, const double* xref,
                               const double* R, const double* foot, const uint8_t* contact, double* grf, double* u_full, double* warm_x, double* warm_y, double* rho,
                               int32_t* iters, int32_t* status, int32_t* nfact) {
    san_modes(twin, contact_stride, carry);
    return a1mpc_emu_solve_split(P, horizon, n, nrows, x0, xref, R, foot, contact, grf, u_full, warm_x, warm_y, rho, iters, status, nfact);
}
extern "C" int san_solve_gen(int twin, double* carry, const a1mpc::DeviceParams* P, int horizon, int n, const double* x0, const double* xref, const double* R,
                             const double* foot, int foot_stride, const uint8_t* contact, int contact_stride, double* grf, double* u_full, double* warm_x, double* warm_y,
                             double* rho, int32_t* iters, int32_t* status, int32_t* nfact) {
    san_modes(twin, 0, carry);
    return a1mpc_emu_solve_gen(P, horizon, n, x0, xref, R, foot, foot_stride, contact, contact_stride, grf, u_full, warm_x, warm_y, rho, iters, status, nfact);
}
extern "C" int san_balance(const a1mpc::DeviceParams* P, int n, const double* root_acc, const double* R, const double* Rz, const double* foot, const uint8_t* contact,
                           double* grf, double* f_world, int32_t* iters, int32_t* status) {
    return a1mpc_emu_balance(P, n, root_acc, R, Rz, foot, contact, grf, f_world, iters, status);
}
'''


def solver_library(horizon):
    """the harness with the `case`s of one horizon, under asan (`#include`d, so that the flags carry the paths; the name carries the hash of everything it includes)"""
    import types
    text = "".join(open(os.path.join(_HERE, f)).read() for f in SOLVER_SOURCES) + "".join(open(os.path.join(_CSRC, f)).read() for f in SOLVER_HEADERS)
    pre = f"// sources {hashlib.sha256(text.encode()).hexdigest()}\n#include \"emu_harness.cpp\"\n"
    module = types.SimpleNamespace(__name__=f"emu_solver_h{horizon}", _PRE=pre, section=lambda: "", _POST=SOLVER_POST)
    return Library(module, "asan", extra_flags=("-I", _HERE, "-I", _CSRC, f"-DA1_EMU_ONLY_H={horizon}"))
