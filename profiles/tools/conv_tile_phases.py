"""Phase clocks of the 256-pixel convolution tile (k_conv_x6r, LDS-DMA weights), from a DIAGNOSTIC build of the library.

    conv_tile_phases.py --build DIR                 compile csrc/*.hip with -DFH_CONV_PHASE_CLOCKS into DIR/libfh_hip.so
    conv_tile_phases.py --lib DIR/libfh_hip.so [--batch 8] [--out FILE.md]
    conv_tile_phases.py                             both, in a temporary directory

With the flag, thread 0 of every workgroup leaves s_memtime at five points of its tile (0 entry, 1 first barrier passed,
2 K loop done, 3 last store issued, 4 group sums reduced and stores retired = exit) and the wave's HW_ID / XCC_ID; the shipped
library has no stamp.  Reported per shape and epilogue form (FH_CONV_TILE_TAIL=0: 4 bytes per lane; default: 16 bytes), as
medians over the tiles of one launch in s_memtime ticks: prologue (0 -> 1), K loop (1 -> 2), epilogue issue (2 -> 3), reduce +
store drain (3 -> 4), and the gap between one workgroup's exit and the entry of the next workgroup on the same CU (grouped
by XCC_ID and the SE / SH / CU bits of HW_ID, ordered by the entry stamp)."""
import ctypes, glob, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(256, 256, 128, 128, "plain"), (256, 256, 128, 128, "res_gn0"), (256, 256, 128, 128, "gn1"),
          (256, 256, 256, 128, "norm"), (128, 128, 256, 256, "plain")]


def build(d):
    d = os.path.abspath(d)
    os.makedirs(d, exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(ROOT, "free-hunch_amd", "csrc", "*.hip")))
    out = os.path.join(d, "libfh_hip.so")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-std=c++17",
                           "-munsafe-fp-atomics", "-DFH_CONV_PHASE_CLOCKS", "-shared", "-fPIC", "-o", out] + srcs,
                          cwd=os.path.join(ROOT, "free-hunch_amd", "csrc"))
    return out


def child(libpath, N):
    sys.path.insert(0, ROOT)
    import torch
    from free_hunch_amd import _lib as L
    L.LIB_PATH = libpath
    lib = L.load(); dev = torch.device("cuda:0"); out = {}
    lib.fh_conv_phase_buffer.argtypes, lib.fh_conv_phase_buffer.restype = [ctypes.c_void_p], ctypes.c_int
    plan = (ctypes.c_int32 * 8)()
    for (H, W, Ci, Co, mode) in SHAPES:
        g = torch.Generator().manual_seed(N + H + Ci + Co)
        x = torch.randn(N, H, W, Ci, generator=g).to(dev)
        wd = (torch.randn(Co, 9, Ci, generator=g) * 0.03).to(dev)
        h = wd.to(torch.bfloat16); r = wd - h.float(); m = r.to(torch.bfloat16); l = (r - m.float()).to(torch.bfloat16)
        wx = torch.stack([h, m, l]).reshape(3, Co, 9, Ci // 32, 32).permute(0, 2, 3, 1, 4).contiguous()
        b = torch.zeros(Co, device=dev); o = torch.empty(N, H, W, Co, device=dev)
        res = torch.randn(N, H, W, Co, generator=g).to(dev) if mode == "res_gn0" else None
        chunks = lib.fh_conv2d_x6_gn_chunks(1, N, H, W, Ci, Co, 3, 3, 1, 1)
        partial = torch.zeros(N * chunks * 64, dtype=torch.float64, device=dev)
        e = L.FhGnEpilogue(); e.partial, e.mode, e.act = partial.data_ptr(), int(mode == "gn1"), 1
        if mode == "gn1":
            xin = torch.randn(N, H, W, Co, generator=g).to(dev); tab = torch.randn(N, 5, Co, generator=g).to(dev)
            e.x, e.tab = xin.data_ptr(), tab.data_ptr()
        table = torch.cat([1 + 0.1 * torch.randn(N, 1, Ci, generator=g), 0.1 * torch.randn(N, 1, Ci, generator=g)], 1).to(dev).contiguous()
        rp = res.data_ptr() if res is not None else None
        if mode == "plain":
            f = lambda: L.check(lib.fh_conv2d_x6_nhwc(x.data_ptr(), wx.data_ptr(), b.data_ptr(), None, o.data_ptr(), None, 1,
                                                      N, H, W, Ci, Co, 3, 3, 1, 1, L.stream()), "x6")
        elif mode == "norm":
            f = lambda: L.check(lib.fh_conv2d_x6_norm_nhwc(x.data_ptr(), table.data_ptr(), 1, wx.data_ptr(), b.data_ptr(), None,
                                                           o.data_ptr(), N, H, W, Ci, Co, L.stream()), "x6 norm")
        else:
            f = lambda: L.check(lib.fh_conv2d_x6_nhwc_gn(x.data_ptr(), wx.data_ptr(), b.data_ptr(), rp, o.data_ptr(), None, 1,
                                                         N, H, W, Ci, Co, 3, 3, 1, 1, ctypes.byref(e), L.stream()), "x6 gn")
        assert lib.fh_conv2d_x6_plan(1, N, H, W, Ci, Co, 3, 3, 1, 1, plan) == 0 and plan[1] == 256
        tiles = plan[5] * plan[6]
        for _ in range(5): f()
        stamps = torch.zeros(tiles, 8, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert lib.fh_conv_phase_buffer(stamps.data_ptr()) == 0
        f(); torch.cuda.synchronize()
        assert lib.fh_conv_phase_buffer(None) == 0
        s = stamps.cpu().tolist()
        assert all(t[0] and t[1] and t[2] and t[3] and t[4] for t in s), "a tile left no stamp"
        med = lambda v: statistics.median(v) if v else None
        row = {"tiles": tiles, "prologue": med([t[1] - t[0] for t in s]), "loop": med([t[2] - t[1] for t in s]),
               "epilogue_issue": med([t[3] - t[2] for t in s]), "store_drain": med([t[4] - t[3] for t in s]),
               "tile": med([t[4] - t[0] for t in s])}
        cus = {}
        for t in s:
            if t[5] or t[6]:
                cus.setdefault((t[6] & 15, (t[5] >> 8) & 255), []).append((t[0], t[4]))
        gaps = []
        for v in cus.values():
            v.sort()
            gaps += [v[i + 1][0] - v[i][1] for i in range(len(v) - 1)]
        row["cus_seen"], row["gap"] = len(cus), med(gaps)
        out["%d,%d,%d,%d,%d,%s" % (N, H, W, Ci, Co, mode)] = row
    print("RESULT " + json.dumps(out), flush=True)


def main(argv):
    opt = {argv[i]: argv[i + 1] for i in range(len(argv) - 1) if argv[i].startswith("--")}
    if "--build" in opt:
        print(build(opt["--build"])); return
    libpath = os.path.abspath(opt["--lib"]) if "--lib" in opt else build(tempfile.mkdtemp(prefix="fh_phase_clocks_"))
    lines = ["median s_memtime ticks per tile over the tiles of one launch, batch %s" % opt.get("--batch", "8"), "",
             "| H x W | Cin | Cout | mode | form | tiles | prologue | K loop | epilogue issue | reduce + store drain | tile | gap to next workgroup | CUs seen |",
             "|---" * 13 + "|"]
    res = {}
    for form, env in (("4-byte epilogue", {"FH_CONV_TILE_TAIL": "0"}), ("16-byte epilogue", {})):
        e = dict(os.environ, **env)
        if not env:
            e.pop("FH_CONV_TILE_TAIL", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", libpath, opt.get("--batch", "8")], env=e,
                           stdout=subprocess.PIPE, text=True, timeout=600, check=True)
        res[form] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for key in next(iter(res.values())):
        _N, H, W, Ci, Co, mode = key.split(",")
        for form in res:
            r = res[form][key]
            lines.append("| %s x %s | %s | %s | %s | %s | %d | %s | %s | %s | %s | %s | %s | %s |" % (
                H, W, Ci, Co, mode, form, r["tiles"], r["prologue"], r["loop"], r["epilogue_issue"], r["store_drain"], r["tile"],
                "-" if r["gap"] is None else r["gap"], r["cus_seen"]))
    print("\n".join(lines))
    if "--out" in opt:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if "--child" in sys.argv:
    i = sys.argv.index("--child"); child(sys.argv[i + 1], int(sys.argv[i + 2]))
else:
    main(sys.argv[1:])
