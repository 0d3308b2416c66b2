#!/usr/bin/env python3
"""K1 A/B experiments (profiling aid): builds libgomoku_hip variants that differ in eval_kernel.hip's -DGMK_K1_* switches only
(the other objects are the production ones) and times them back to back on the same box.
usage: k1_variants.py build name=FLAG,FLAG ...   (in the container; writes gomokuai_amd/var/libgomoku_hip_<name>.so)
       k1_variants.py run [name ...]             (on the GPU box; prints ms per launch of the 65 536-board batch, 3 rounds interleaved)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VAR = os.path.join(ROOT, "gomokuai_amd", "var")


def build(specs):
    from gomokuai_amd import build as B
    B.build_lib()
    os.makedirs(VAR, exist_ok=True)
    source = os.environ.get("GMK_VARIANT_SOURCE", "eval_kernel.hip")       # (the same harness for another kernel file's -D switches)
    others = [os.path.join(B.CSRC, os.path.splitext(s)[0] + ".o") for s in B.LIB_SOURCES if s != source]
    procs = []
    for spec in specs:
        name, _, flags = spec.partition("=")
        obj = os.path.join(VAR, "%s_%s.o" % (os.path.splitext(source)[0], name))
        cmd = [B.HIPCC] + B.FLAGS + ["-D" + f for f in flags.split(",") if f] + ["-x", "hip", "-c", os.path.join(B.CSRC, source), "-o", obj]
        procs.append((name, obj, subprocess.Popen(cmd)))
    for name, obj, p in procs:
        if p.wait() != 0:
            raise SystemExit("variant %s failed to compile" % name)
        subprocess.check_call([B.HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", os.path.join(VAR, "libgomoku_hip_%s.so" % name), obj] + others)
        print("built", name)


def run(names):
    names = names or sorted(f[len("libgomoku_hip_"):-3] for f in os.listdir(VAR) if f.endswith(".so"))
    results = {n: [] for n in names}
    sums = {}
    for rnd in range(3):
        for n in names:
            env = dict(os.environ, GMK_HIP_LIB=os.path.join(VAR, "libgomoku_hip_%s.so" % n), GMK_EVAL_REPS="200")
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_time.py"), "all", "check"], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in out.stdout.splitlines() if l.startswith("all")]
            if not line:
                print(n, "FAILED", out.stdout[-300:], out.stderr[-600:]); results[n].append(float("nan")); continue
            results[n].append(float(line[0].split()[1]))
            sums.setdefault(n, set()).update(l.split()[1] for l in out.stdout.splitlines() if l.startswith("checksum"))
    ref = sums.get("base")
    for n in names:
        print("%-24s %s   min %.4f   %s" % (n, "  ".join("%.4f" % x for x in results[n]), min(results[n]),
                                            "" if ref is None else ("outputs = base" if sums.get(n) == ref else "OUTPUTS DIFFER FROM base: %s" % sums.get(n))))


def one_process(names, rounds=9, launches=300):
    """every build's library loaded into THIS process (separate copies: separate paths), `rounds` rounds of `launches` event-timed launches each, the builds
    taken in turn within a round and the turn order rotated from round to round; the four outputs of every build compared with the first build's, word for word"""
    import ctypes as C
    import numpy as np, torch
    from gomokuai_amd import lib as G
    names = names or sorted(f[len("libgomoku_hip_"):-3] for f in os.listdir(VAR) if f.endswith(".so"))
    n = int(os.environ.get("GMK_EVAL_BOARDS", "65536"))
    torch.cuda.set_device(0); G.init(0)
    _, _, planes = G.synth_boards(n, int(os.environ.get("GMK_EVAL_KIND", "0")))
    dev = torch.device("cuda", 0)
    d_planes = torch.from_numpy(planes.view(np.int16).reshape(n, 32)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    libs, outs = {}, {}
    for name in names:
        L = C.CDLL(os.path.join(VAR, "libgomoku_hip_%s.so" % name))
        L.gmk_init.argtypes = [C.c_int]
        L.gmk_eval_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        if L.gmk_init(0) < 0:
            raise SystemExit("%s: gmk_init failed" % name)
        libs[name] = L
        outs[name] = [torch.full((n, w), 0x5A5A5A5A, dtype=torch.int32, device=dev) for w in (900, 900, 11, 1)]

    def launch(name):
        o = outs[name]
        if libs[name].gmk_eval_batch(d_planes.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), stream) < 0:
            raise SystemExit("%s: gmk_eval_batch failed" % name)

    for name in names:
        for _ in range(10): launch(name)
    torch.cuda.synchronize()
    same = {name: all(torch.equal(a, b) for a, b in zip(outs[names[0]], outs[name])) for name in names}
    times = {name: [] for name in names}
    for rnd in range(rounds):
        for k in range(len(names)):
            name = names[(k + rnd) % len(names)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches): launch(name)
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / launches)
    ref = sorted(times[names[0]])[rounds // 2]
    for name in names:
        t = sorted(times[name])
        print("%-12s %s   median %.4f  min %.4f  max %.4f  (%+.2f %% of %s's median)   outputs %s" % (name, " ".join("%.4f" % x for x in times[name]), t[rounds // 2], t[0], t[-1],
              100.0 * (t[rounds // 2] / ref - 1.0), names[0], "= %s's" % names[0] if same[name] else "DIFFER FROM %s's" % names[0]), flush=True)
    if not all(same.values()):
        raise SystemExit(1)


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build(sys.argv[2:])
    elif sys.argv[1] == "oneproc":       # (on the GPU box: ms per launch, every build in one process)
        one_process(sys.argv[2:])
    else:
        run(sys.argv[2:])
