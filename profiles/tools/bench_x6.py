"""Timings of the split-bf16 convolution (fh_conv2d_x6_nhwc).

    bench_x6.py                      accuracy against float64 and time against the fp32-MFMA convolution, a few large shapes
    bench_x6.py --splitk [--batches 4,8] [--parent-root DIR] [--variants NAME=ENV=VAL,...] [--out FILE.json]
        A/B of the split-K launches of the FFHQ-256 network's 3 x 3 layers that the plan sends to the row-reuse kernel:
        every variant is a child process (the switch FH_CONV_SPLITK_REUSE is read once per process) timing each layer shape
        with events on the stream, REPEATS repeats of LAUNCHES launches.  The generic kernel (switch off) runs first AND
        last; its spread per shape is max - min over the repeats of both runs, and a gain counts where the medians differ by
        more than that.  --parent-root: another checkout (built) whose library is timed as well.
    bench_x6.py --tile-tail [--batches 4,8] [--parent-root DIR] [--out FILE.json]
        A/B of the 16-byte epilogue of the 256-pixel tiles (switch FH_CONV_TILE_TAIL) on five launches of the 256^2 and
        128^2 levels - plain, residual + group sums, backward group sums, fused GroupNorm input - by the same method.
"""
import json, os, statistics, subprocess, sys
ROOT=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPEATS, LAUNCHES = 7, 100


def splitk_child(root, shapes_file):
    """times every (N, H, W, Ci, Co, ks) of the file with the library of checkout `root` -> JSON {key: [us per launch] * REPEATS}"""
    sys.path.insert(0, root)
    import torch
    from free_hunch_amd import _lib as L
    lib = L.load(); dev = torch.device('cuda:0'); out = {}
    for (N, H, W, Ci, Co, ks) in json.load(open(shapes_file)):
        g = torch.Generator().manual_seed(N + H + Ci + Co)
        x = torch.randn(N, H, W, Ci, generator=g).to(dev)
        wd = (torch.randn(Co, 9, Ci, generator=g) * 0.03).to(dev)
        h = wd.to(torch.bfloat16); r = wd - h.float(); m = r.to(torch.bfloat16); l = (r - m.float()).to(torch.bfloat16)
        wx = torch.stack([h, m, l]).reshape(3, Co, 9, Ci // 32, 32).permute(0, 2, 3, 1, 4).contiguous()
        b = torch.zeros(Co, device=dev); o = torch.empty(N, H, W, Co, device=dev); ws = torch.empty(ks, N * H * W, Co, device=dev)
        f = lambda: L.check(lib.fh_conv2d_x6_nhwc(x.data_ptr(), wx.data_ptr(), b.data_ptr(), None, o.data_ptr(), ws.data_ptr(), ks,
                                                  N, H, W, Ci, Co, 3, 3, 1, 1, L.stream()), "x6")
        for _ in range(10): f()
        ts = []
        for _ in range(REPEATS):
            torch.cuda.synchronize(); e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES): f()
            e1.record(); torch.cuda.synchronize(); ts.append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
        out["%d,%d,%d,%d,%d,%d" % (N, H, W, Ci, Co, ks)] = ts
    print("RESULT " + json.dumps(out), flush=True)


def splitk_main(argv):
    import ctypes
    opt = {argv[i]: argv[i + 1] for i in range(len(argv) - 1) if argv[i].startswith("--")}
    batches = [int(v) for v in opt.get("--batches", "4,8").split(",")]
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
    import make_conv_plan
    from free_hunch_amd import _lib as L, unet
    lib = L.load(); buf = (ctypes.c_int32 * 8)()
    shapes = []
    for N in batches:
        for H, W, Ci, Co, k, stride in make_conv_plan.unet_layers(unet.FFHQ256, unet._plan):
            ks = lib.fh_conv2d_splitk(N, H, W, Ci, Co, k, k)
            if ks > 1 and lib.fh_conv2d_x6_plan(ks, N, H, W, Ci, Co, k, k, k // 2, stride, buf) == 0 and buf[0] == 2:
                shapes.append((N, H, W, Ci, Co, ks))
    import tempfile
    fd, sf = tempfile.mkstemp(suffix=".json", prefix="bench_x6_splitk_shapes_")
    with os.fdopen(fd, "w") as f:
        json.dump(shapes, f)
    variants = [("generic_first", ROOT, {"FH_CONV_SPLITK_REUSE": "0"}), ("reuse", ROOT, {})]
    for spec in filter(None, opt.get("--variants", "").split(",")):
        name, key, val = spec.split("=")
        variants.append((name, ROOT, {key: val}))
    if "--parent-root" in opt:
        variants.append(("parent", os.path.abspath(opt["--parent-root"]), {}))
    variants.append(("generic_last", ROOT, {"FH_CONV_SPLITK_REUSE": "0"}))
    res = {}
    for name, root, env in variants:
        e = dict(os.environ, **env)
        if not env:
            e.pop("FH_CONV_SPLITK_REUSE", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--splitk-child", root, sf], env=e, stdout=subprocess.PIPE,
                           text=True, timeout=600, check=True)
        res[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print("ran", name, flush=True)
    others = [n for n, _r, _e in variants if not n.startswith("generic")]
    print("us per call (split-K kernel + reduce), median of %d x %d launches; spread = max - min of the generic kernel's %d repeats"
          % (REPEATS, LAUNCHES, 2 * REPEATS))
    print("| N | H x W | Cin | Cout | ksplit | generic | spread | " + " | ".join("%s | gain" % n for n in others) + " |")
    print("|---" * (7 + 2 * len(others)) + "|")
    tot = {}
    for N, H, W, Ci, Co, ks in shapes:
        key = "%d,%d,%d,%d,%d,%d" % (N, H, W, Ci, Co, ks)
        gen = res["generic_first"][key] + res["generic_last"][key]
        gm, sp = statistics.median(gen), max(gen) - min(gen)
        cells = []
        t = tot.setdefault((N, W), {"generic": 0.0, "spread": 0.0, "shapes": 0})
        t["generic"] += gm; t["spread"] += sp; t["shapes"] += 1
        for n in others:
            m = statistics.median(res[n][key])
            t[n] = t.get(n, 0.0) + m
            gain = gm - m
            cells.append("%.1f | %+.1f%s" % (m, gain, " *" if abs(gain) > sp else ""))
        print("| %d | %d x %d | %d | %d | %d | %.1f | %.1f | %s |" % (N, H, W, Ci, Co, ks, gm, sp, " | ".join(cells)))
    print("\nper batch and width, summed over its shapes (one launch each); * = beyond the summed spread")
    print("| N | W | shapes | generic | spread | " + " | ".join("%s | gain" % n for n in others) + " |")
    print("|---" * (5 + 2 * len(others)) + "|")
    for (N, W), t in sorted(tot.items()):
        cells = ["%.1f | %+.1f (%+.1f %%)%s" % (t[n], t["generic"] - t[n], 100 * (t["generic"] - t[n]) / t["generic"],
                                              " *" if abs(t["generic"] - t[n]) > t["spread"] else "") for n in others]
        print("| %d | %d | %d | %.1f | %.1f | %s |" % (N, W, t["shapes"], t["generic"], t["spread"], " | ".join(cells)))
    os.remove(sf)
    if "--out" in opt:
        json.dump({"shapes": shapes, "repeats": REPEATS, "launches": LAUNCHES, "us_per_call": res}, open(opt["--out"], "w"))


TAIL_SHAPES = [(256, 256, 128, 128, "plain"), (256, 256, 128, 128, "res_gn0"), (256, 256, 128, 128, "gn1"),
               (256, 256, 256, 128, "norm"), (128, 128, 256, 256, "plain")]


def tail_child(root, batches):
    """times the five 256-pixel-tile launches of --tile-tail with the library of checkout `root`"""
    import ctypes
    sys.path.insert(0, root)
    import torch
    from free_hunch_amd import _lib as L
    lib = L.load(); dev = torch.device('cuda:0'); out = {}
    for N in [int(v) for v in batches.split(",")]:
        for (H, W, Ci, Co, mode) in TAIL_SHAPES:
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
            for _ in range(10): f()
            ts = []
            for _ in range(REPEATS):
                torch.cuda.synchronize(); e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LAUNCHES): f()
                e1.record(); torch.cuda.synchronize(); ts.append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
            out["%d,%d,%d,%d,%d,%s" % (N, H, W, Ci, Co, mode)] = ts
    print("RESULT " + json.dumps(out), flush=True)


def tail_main(argv):
    """--tile-tail [--batches 4,8] [--parent-root DIR] [--out FILE.json]: A/B of the 16-byte epilogue of the 256-pixel tiles.
    The parent form (the library of --parent-root, else this one with FH_CONV_TILE_TAIL=0) runs first and last, between them
    this library with the switch off (the 4-byte epilogue it keeps) and with the default; every variant is a child process.
    Spread = max - min of the parent form's 2 x REPEATS repeats; * marks a gain beyond it."""
    opt = {argv[i]: argv[i + 1] for i in range(len(argv) - 1) if argv[i].startswith("--")}
    batches = opt.get("--batches", "4,8")
    proot = os.path.abspath(opt["--parent-root"]) if "--parent-root" in opt else ROOT
    variants = [("parent_first", proot, {"FH_CONV_TILE_TAIL": "0"}), ("switch_off", ROOT, {"FH_CONV_TILE_TAIL": "0"}),
                ("epilogue16", ROOT, {}), ("parent_last", proot, {"FH_CONV_TILE_TAIL": "0"})]
    res = {}
    for name, root, env in variants:
        e = dict(os.environ, **env)
        if not env:
            e.pop("FH_CONV_TILE_TAIL", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tile-tail-child", root, batches], env=e,
                           stdout=subprocess.PIPE, text=True, timeout=600, check=True)
        res[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print("ran", name, flush=True)
    print("us per launch, median of %d x %d launches; spread = max - min of the parent form's %d repeats" % (REPEATS, LAUNCHES, 2 * REPEATS))
    print("| N | H x W | Cin | Cout | mode | parent | spread | switch off | gain | 16-byte epilogue | gain |")
    print("|---" * 11 + "|")
    for key in res["parent_first"]:
        par = res["parent_first"][key] + res["parent_last"][key]
        pm, sp = statistics.median(par), max(par) - min(par)
        cells = []
        for n in ("switch_off", "epilogue16"):
            m = statistics.median(res[n][key])
            cells.append("%.1f | %+.1f (%+.1f %%)%s" % (m, pm - m, 100 * (pm - m) / pm, " *" if pm - m > sp else ""))
        N, H, W, Ci, Co, mode = key.split(",")
        print("| %s | %s x %s | %s | %s | %s | %.1f | %.1f | %s |" % (N, H, W, Ci, Co, mode, pm, sp, " | ".join(cells)))
    if "--out" in opt:
        json.dump({"repeats": REPEATS, "launches": LAUNCHES, "us_per_launch": res}, open(opt["--out"], "w"))


if "--tile-tail-child" in sys.argv:
    tail_child(*sys.argv[sys.argv.index("--tile-tail-child") + 1:][:2]); sys.exit(0)
if "--tile-tail" in sys.argv:
    tail_main(sys.argv[1:]); sys.exit(0)
if "--splitk-child" in sys.argv:
    splitk_child(*sys.argv[sys.argv.index("--splitk-child") + 1:][:2]); sys.exit(0)
if "--splitk" in sys.argv:
    splitk_main(sys.argv[1:]); sys.exit(0)

import torch, math
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT,'tests')); sys.path.insert(0, os.path.join(ROOT,'tests','golden'))
from free_hunch_amd import _lib as L
from test_hip_unet import wino_weights
lib=L.load(); dev=torch.device('cuda:0')
def split_w(wd):
    h=wd.to(torch.bfloat16); r=wd-h.float(); m=r.to(torch.bfloat16); r=r-m.float(); l=r.to(torch.bfloat16)
    Co,T,Ci=wd.shape
    return torch.stack([h,m,l]).reshape(3,Co,T,Ci//32,32).permute(0,2,3,1,4).contiguous()
# accuracy vs float64
torch.manual_seed(0)
for (N,H,W,Ci,Co) in [(1,32,32,128,128),(2,16,16,512,256)]:
    x=torch.randn(N,H,W,Ci,device=dev)*torch.rand(N,H,W,Ci,device=dev)*3; w=torch.randn(Co,Ci,3,3,device=dev)*0.05; b=torch.randn(Co,device=dev)
    ref=torch.nn.functional.conv2d(x.permute(0,3,1,2).double(), w.double(), b.double(), padding=1).permute(0,2,3,1)
    wd=w.permute(0,2,3,1).reshape(Co,9,Ci).contiguous(); wx=split_w(wd); wu=wino_weights(w)
    out=torch.empty(N,H,W,Co,device=dev)
    errs={}
    L.check(lib.fh_conv2d_nhwc(x.data_ptr(),wd.data_ptr(),b.data_ptr(),None,out.data_ptr(),None,1,N,H,W,Ci,Co,3,3,1,1,L.stream()),"c"); errs['f32 mfma']=float((out.double()-ref).abs().max())
    L.check(lib.fh_conv3x3_wino_nhwc(x.data_ptr(),wu.data_ptr(),b.data_ptr(),None,out.data_ptr(),N,H,W,Ci,Co,L.stream()),"w"); errs['wino f32']=float((out.double()-ref).abs().max())
    out.zero_()
    L.check(lib.fh_conv2d_x6_nhwc(x.data_ptr(),wx.data_ptr(),b.data_ptr(),None,out.data_ptr(),None,1,N,H,W,Ci,Co,3,3,1,1,L.stream()),"x"); errs['bf16x6']=float((out.double()-ref).abs().max())
    t32=torch.nn.functional.conv2d(x.permute(0,3,1,2), w, b, padding=1).permute(0,2,3,1); errs['torch f32 (MIOpen)']=float((t32.double()-ref).abs().max())
    print((N,H,W,Ci,Co), "ref max %.2f"%float(ref.abs().max()), {k:"%.2e"%v for k,v in errs.items()}, flush=True)
shapes=[(8,256,256,128,128),(8,256,256,256,128),(8,128,128,256,256),(8,64,64,256,256),(1,256,256,128,128),(8,32,32,256,256),(8,16,16,512,512),(8,8,8,512,512)]
for (N,H,W,Ci,Co) in shapes:
    x=torch.randn(N,H,W,Ci,device=dev); w=torch.randn(Co,Ci,3,3,device=dev)*0.03; b=torch.zeros(Co,device=dev); out=torch.empty(N,H,W,Co,device=dev)
    wd=w.permute(0,2,3,1).reshape(Co,9,Ci).contiguous(); wx=split_w(wd)
    ks=lib.fh_conv2d_splitk(N,H,W,Ci,Co,3,3); ws=torch.empty(max(ks,1),N*H*W,Co,device=dev)
    f1=lambda: L.check(lib.fh_conv2d_x6_nhwc(x.data_ptr(),wx.data_ptr(),b.data_ptr(),None,out.data_ptr(),ws.data_ptr(),ks,N,H,W,Ci,Co,3,3,1,1,L.stream()),"x")
    f2=lambda: L.check(lib.fh_conv2d_nhwc(x.data_ptr(),wd.data_ptr(),b.data_ptr(),None,out.data_ptr(),ws.data_ptr(),ks,N,H,W,Ci,Co,3,3,1,1,L.stream()),"c")
    res=[]
    for f in (f1,f2):
        for _ in range(3): f()
        torch.cuda.synchronize(); e0=torch.cuda.Event(enable_timing=True); e1=torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10): f()
        e1.record(); torch.cuda.synchronize(); res.append(e0.elapsed_time(e1)/10)
    fl=2.0*N*H*W*Ci*Co*9
    print("N%d %3dx%-3d Ci%4d Co%4d ks%d: x6 %7.3f ms (%5.1f fp32-equiv TF/s)   direct f32 %7.3f ms (%5.1f TF/s)  speedup %.2f" % (N,H,W,Ci,Co,ks,res[0],fl/res[0]/1e9,res[1],fl/res[1]/1e9,res[1]/res[0]), flush=True)
