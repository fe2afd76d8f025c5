"""The conv plan (csrc/conv_plan.h: which kernel runs where, its grid, stats rows and workspace) without a GPU.

csrc/conv_plan.cpp and a thin driver (tests/native/conv_plan_main.cpp) are built with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer -- plain C++, no HIP -- and fed shapes on stdin, with the A/B knobs unset:

  * every plan's stats rows stay within conv_stats_rows, the bound conv_fwd checks the slab against before it
    launches (a wrong bound is an out-of-bounds write);
  * a plan offered conv_ws_elems elements uses no more;
  * a forced kernel yields that kernel or "unsupported", never another one;
  * every forward / eval case of tests/lattice.py plans to the kernel its `pref` names;
  * the auto dispatch of the 256^2 U-Net's conv layers (training forward and input gradients at batch 64 and 4,
    eval at N = 1 and 4) is pinned to the kernels of a kernel trace taken before the plan existed
    (profiles/conv_dispatch.md): the thresholds behind it are measured decisions.
"""
import os
import shutil
import subprocess

import pytest

import lattice as L
from robotic_discovery_platform_amd.models.unet import unet_conv_specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RDP_ROWBAND", "RDP_ROWBAND_X_MAXPIX", "RDP_ROWBAND_R2", "RDP_PP_SPLIT", "RDP_SPLITK_BNRED")
KERNELS = ("AUTO", "HALO", "IGEMM8_128", "IGEMM8_256", "PP256", "PP128", "RING", "PPSK128", "PPSK256", "FIRST", "RING2",
           "RING2X2", "ROWBAND", "IGEMM4_128", "IGEMM4_256")
INT_KEYS = ("code", "bm", "bn", "waves", "ksplit", "mode", "launches", "grid", "rgrid", "rows", "ws", "pool", "up",
            "bnrows", "bound", "need")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("conv_plan") / "conv_plan_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "csrc"), os.path.join(ROOT, "csrc", "conv_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "conv_plan_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr
    return exe


def _run(exe, lines, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    env.update(ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for ln in r.stdout.splitlines():
        d = dict(kv.split("=", 1) for kv in ln.split())
        out.append({k: (int(v) if k in INT_KEYS else v) for k, v in d.items()})
    assert len(out) == len(lines)
    return out


def _plan(n, h, w, c1, c2, cout, kernel="AUTO", taps=9, packed=0, stats=0, ev=0, split=0, ws=0, pool=0, up=0, bn=0,
          wfrag=0, bnin=0):
    return (f"plan {n} {h} {w} {c1} {c2} {cout} {taps} {int(packed)} {kernel} {int(stats)} {int(ev)} {split} {ws} "
            f"{int(pool)} {int(up)} {int(bn)} {int(wfrag)} {int(bnin)}")


# ---------------------------------------------------------------------------------------------
# the U-Net's convs as the executor issues them (models/unet.py): forward, eval, input gradients
# ---------------------------------------------------------------------------------------------

def _unet_layers(size, bilinear=True):
    """(name, map side, c1, c2, cout, packed, pool after, upsample after) per conv layer, forward order."""
    specs = unet_conv_specs(4, 64, 3, bilinear)
    out = []
    for i, sp in enumerate(specs):
        blk = i // 2                       # inc, down1..4, up1..4
        lvl = blk if blk <= 4 else 8 - blk
        s = size >> lvl
        c1, c2 = (8, 0) if sp.packed else (sp.cin, 0)
        if blk > 4 and i % 2 == 0:         # first conv of an Up block reads cat(skip, upsampled)
            c1 = c2 = sp.cin // 2
        second = i % 2 == 1
        out.append((sp.name, s, c1, c2, sp.cout, sp.packed, second and blk < 4, second and 4 <= blk < 8))
    return out


def _fwd_queries(n, size, ev, ws):
    q = []
    for _, s, c1, c2, cout, packed, pool, up in _unet_layers(size):
        q.append(_plan(n, s, s, c1, c2, cout, packed=packed, stats=not ev, ev=ev, ws=ws, pool=ev and pool,
                       up=ev and up, wfrag=ev and not packed))
    return q


def _dgrad_queries(n, size, ws, owned_only=False):
    """owned_only: the BN-backward operand as the executor offers it, only where dx is the activation gradient of a
    BN layer -- the second conv of a block, whose input is the first conv's activation (the other input gradients
    go to a pool or to the concat's halves)."""
    q = []
    for i, (_, s, c1, c2, cout, packed, _, _) in enumerate(_unet_layers(size)):
        if not packed:  # dy (cout channels) -> d(input), split over the concat's two sources
            q.append(_plan(n, s, s, cout, 0, c1 + c2, split=c1 if c2 else 0, ws=ws, bn=i % 2 == 1 or not owned_only))
    return q


def _unet_ws(exe, n, size, training):
    """The executor's shared split-K workspace: the largest conv_ws_elems of its convs."""
    lines = []
    for _, s, c1, c2, cout, packed, _, _ in _unet_layers(size):
        lines.append(f"ws {n} {s} {s} {c1} {c2} {cout} 9 {int(packed)} AUTO")
        if training and not packed:
            lines.append(f"ws {n} {s} {s} {cout} 0 {c1 + c2} 9 0 AUTO")
    return max(int(d["ws"]) for d in _run(exe, lines))


# The kernels of the parent commit's kernel traces (one 256^2 training step at batch 64 and at batch 4, one eval
# forward at N = 1 and N = 4), per conv layer in forward order: inc 1-2, down1..4 1-2, up1..4 1-2. RING2X2 shows in a
# trace as two RING2 launches. The input gradients skip the first layer.
PINNED = {
    ("train", 64): ["FIRST", "RING", "RING", "RING2X2", "PP256", "PP256", "PP256", "PP256", "PP128", "PP128",
                    "PP256", "PP256", "PP256", "PP128", "PP128", "RING2", "RING2", "RING"],
    ("dgrad", 64): ["RING", "RING2", "RING2X2", "PP128", "PP256", "PP256", "PP256", "PP128", "PP128",
                    "PP256", "PP256", "PP256", "PP256", "PP256", "RING", "RING", "RING"],
    ("train", 4): ["FIRST", "RING", "RING", "PP128", "IGEMM8_128", "IGEMM8_128", "PPSK128", "PPSK128", "IGEMM8_128",
                   "IGEMM8_128", "PPSK128", "PPSK128", "IGEMM8_128", "PPSK128", "PP128", "RING2", "RING2", "RING"],
    ("dgrad", 4): ["RING", "RING2", "PP128", "PPSK128", "IGEMM8_128", "PPSK128", "PPSK128", "IGEMM8_128", "IGEMM8_128",
                   "IGEMM8_128", "PPSK128", "PP128", "IGEMM8_128", "PP256", "RING", "RING", "RING"],
    ("eval", 1): ["FIRST", "RING", "IGEMM8_128"] + ["ROWBAND"] * 13 + ["RING2", "RING"],
    ("eval", 4): ["FIRST", "RING", "RING", "IGEMM8_128", "IGEMM8_128", "IGEMM8_128", "ROWBAND", "PPSK128", "ROWBAND",
                  "ROWBAND", "PPSK128", "ROWBAND", "IGEMM8_128", "ROWBAND", "IGEMM8_128", "IGEMM8_256", "RING2", "RING"],
}


@pytest.mark.parametrize("mode,n", sorted(PINNED))
def test_unet_auto_dispatch_is_pinned(driver, mode, n):
    ws = _unet_ws(driver, n, 256, mode != "eval")
    q = _dgrad_queries(n, 256, ws) if mode == "dgrad" else _fwd_queries(n, 256, mode == "eval", ws)
    got = [d["kernel"] for d in _run(driver, q)]
    names = [l[0] for l in _unet_layers(256)][1 if mode == "dgrad" else 0:]
    assert got == PINNED[(mode, n)], [(a, g, e) for a, g, e in zip(names, got, PINNED[(mode, n)]) if g != e]


# Where the BN layer that owns each input gradient gets its BN-backward partial rows, from kernel traces of the last
# commit that chose the dgrad binding in Python (one 256^2 training step at batch 64 and at batch 4, bilinear decoder;
# profiles/conv_fused_dispatch.md section 2): "ring" = the dgrad is conv_ring_kernel<64, true, ...>, the BNRED
# instantiation, and bn_bwd_finalize follows it; "splitk" = the dgrad's conv_splitk_reduce_kernel is followed by
# bn_bwd_finalize directly; "pass" = a bn_relu_bwd_reduce / maxpool2_bwd_bn_reduce / upsample2_bwd kernel runs in
# between (also every input gradient no BN layer owns). Same order as PINNED[("dgrad", n)].
BN_ROWS_FROM = {
    64: ["ring"] + ["pass"] * 15 + ["ring"],
    4: ["ring", "pass", "pass", "pass", "pass", "pass", "splitk", "pass", "splitk", "pass", "splitk",
        "pass", "pass", "pass", "pass", "pass", "ring"],
}


@pytest.mark.parametrize("n", sorted(BN_ROWS_FROM))
def test_unet_dgrad_bn_rows_are_pinned(driver, n):
    ws = _unet_ws(driver, n, 256, True)
    got = []
    for p in _run(driver, _dgrad_queries(n, 256, ws, owned_only=True)):
        ring = (p["kernel"], p["form"]) == ("RING", "BNRED")
        assert ring == (p["kernel"] == "RING" and p["bnrows"] > 0), p
        assert p["bnrows"] == 0 or ring or p["ksplit"] > 1, p
        got.append("ring" if ring else "splitk" if p["bnrows"] else "pass")
    names = [l[0] for l in _unet_layers(256)][1:]
    assert got == BN_ROWS_FROM[n], [(a, g, e) for a, g, e in zip(names, got, BN_ROWS_FROM[n]) if g != e]


# ---------------------------------------------------------------------------------------------
# the sweep: bound, workspace, forced kernels
# ---------------------------------------------------------------------------------------------

def _sweep_shapes():
    maps = set()
    for side in ((256, 256), (64, 96), (224, 224), (48, 80)):  # every map of the 5-level pyramid
        for lvl in range(5):
            maps.add((side[0] >> lvl, side[1] >> lvl))
    chans = set()
    for bilinear in (True, False):
        for _, _, c1, c2, cout, packed, _, _ in _unet_layers(256, bilinear):
            chans.add((c1, c2, cout, int(packed), 0))
            if not packed:
                chans.add((cout, 0, c1 + c2, 0, c1 if c2 else 0))  # its input gradient
    for c in L.FWD_CASES + L.EVAL_CASES:
        maps.add((c.H, c.W))
        if c.taps == 9:
            chans.add((c.C1, c.C2, c.Cout, int(c.packed), c.split))
    for c in L.DGRAD_CASES:
        maps.add((c.H, c.W))
        chans.add((c.Cdy, 0, c.Cs + c.Cu, 0, c.Cs))
    return sorted(maps), sorted(chans)


def test_sweep_bound_workspace_forced(driver):
    maps, chans = _sweep_shapes()
    forms = (dict(stats=1), dict(ev=1, pool=1, wfrag=1), dict(ev=1, up=1), dict(bn=1), dict(stats=1, bnin=1))
    lines, req = [], []
    for n in (1, 2, 3, 4, 64):
        for h, w in maps:
            for c1, c2, cout, packed, split in chans:
                for k in KERNELS:
                    for f in forms:
                        if split and ("stats" in f or "ev" in f):
                            continue  # two destinations: the input-gradient form only
                        lines.append(_plan(n, h, w, c1, c2, cout, k, packed=packed, split=split, ws=-1, **f))
                        req.append(k)
    plans = _run(driver, lines)
    bad_bound, bad_ws, bad_forced = [], [], []
    seen = set()
    for ln, k, p in zip(lines, req, plans):
        if p["kernel"] == "UNSUPPORTED":
            continue
        seen.add(p["kernel"])
        if p["rows"] > p["bound"]:
            bad_bound.append((ln, p["kernel"], p["rows"], p["bound"]))
        if p["ws"] > p["need"]:
            bad_ws.append((ln, p["kernel"], p["ws"], p["need"]))
        if p["kernel"] == "AUTO" or (k != "AUTO" and p["kernel"] != k):
            bad_forced.append((ln, p["kernel"]))
    print(f"{len(lines)} plans, {sum(p['kernel'] != 'UNSUPPORTED' for p in plans)} supported")
    assert set(KERNELS) - {"AUTO"} <= seen, "the sweep never reached " + str(set(KERNELS) - {"AUTO"} - seen)
    assert not bad_forced, bad_forced[:5]
    assert not bad_ws, bad_ws[:5]
    assert not bad_bound, (len(bad_bound), bad_bound[:5])


def _ring_fits(c1, c2, cout, split, h, w):
    """The old chain's condition for the ring's fused forms: 64 -> 64, one source, one destination, whole 64-pixel
    row segments, an even number of rows (dense 3x3 weights; none of the sweep's tensors reaches 2 GiB here)."""
    return c1 == 64 and c2 == 0 and cout == 64 and not split and w % 64 == 0 and h % 2 == 0


def test_fused_forms_follow_the_old_chain(driver):
    """The chain of three bindings the plan replaced, transcribed. Input gradients: the BNRED ring wherever it fit, at
    any grid size; else the automatic choice, whose split-K reduce wrote the rows where the conv split K; else the
    plain conv. Forward on a pre-BN input: the BNIN ring or nothing."""
    maps, chans = _sweep_shapes()
    shapes = [(n, h, w) + c for n in (1, 2, 3, 4, 64) for h, w in maps for c in chans
              if not c[3] and n * h * w * max(c[0], c[1], c[2]) * 2 < (1 << 31)]
    q = {}
    for key, kw in (("bn", dict(bn=1)), ("plain", {}), ("ring", dict(kernel="RING")), ("bnin", dict(stats=1, bnin=1)),
                    ("bn_noknob", dict(bn=1))):
        lines = [_plan(n, h, w, c1, c2, cout, split=split, ws=-1, **{k: v for k, v in kw.items()})
                 for n, h, w, c1, c2, cout, _, split in shapes if not (split and "stats" in kw)]
        knobs = dict(RDP_SPLITK_BNRED="0") if key == "bn_noknob" else {}
        q[key] = iter(_run(driver, lines, **knobs))
    same = ("kernel", "grid", "ksplit", "rgrid", "ws", "launches")
    n_ring = n_splitk = 0
    for n, h, w, c1, c2, cout, _, split in shapes:
        bn, plain, forced, off = next(q["bn"]), next(q["plain"]), next(q["ring"]), next(q["bn_noknob"])
        fits = _ring_fits(c1, c2, cout, split, h, w)
        where = (n, h, w, c1, c2, cout, split)
        if fits:
            assert (bn["kernel"], bn["form"]) == ("RING", "BNRED"), (where, bn)
            assert bn["bnrows"] == bn["rows"] == forced["rows"] > 0 and bn["grid"] == forced["grid"], (where, bn, forced)
            assert off == bn, (where, off)  # the knob does not touch the ring form
            n_ring += 1
        else:
            assert bn["form"] != "BNRED" and all(bn[k] == plain[k] for k in same), (where, bn, plain)
            assert bn["bnrows"] in (0, bn["rows"]) and (bn["bnrows"] == 0 or bn["ksplit"] > 1), (where, bn)
            assert off["bnrows"] == 0 and all(off[k] == plain[k] for k in same), (where, off)
            n_splitk += bn["bnrows"] > 0
        if not split:
            bnin = next(q["bnin"])
            assert (bnin["kernel"], bnin["form"]) == (("RING", "BNIN") if fits else ("UNSUPPORTED", "-")), (where, bnin)
            if fits:
                assert bnin["rows"] == forced["rows"] and bnin["grid"] == forced["grid"], (where, bnin, forced)
    assert n_ring > 20 and n_splitk > 20, (n_ring, n_splitk)


def test_unknown_kernel_is_unsupported(driver):
    """A value that is not an enumerator (the retired blocks-per-CU codes among them) is an error."""
    plans = _run(driver, [_plan(2, 9, 13, 64, 64, 128, k, stats=1) for k in ("1000", "2128", "9", "17", "-1", "AUTO")])
    assert [p["kernel"] for p in plans[:-1]] == ["UNSUPPORTED"] * 5 and plans[-1]["kernel"] == "IGEMM8_128"


# ---------------------------------------------------------------------------------------------
# the lattice cases run on the kernel they name
# ---------------------------------------------------------------------------------------------

def test_lattice_cases_plan_to_their_kernel(driver):
    cases = L.FWD_CASES + L.EVAL_CASES
    lines = [_plan(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.pref, taps=c.taps, packed=c.packed, stats=c.stats,
                   ev=c.evalmode, split=c.split, ws=-1 if c.ws else 0, pool=c.pool, wfrag=c.wfrag) for c in cases]
    lines += [_plan(c.N, c.H, c.W, c.Cdy, 0, c.Cs + c.Cu, c.pref, split=c.Cs, ws=-1 if c.ws else 0)
              for c in L.DGRAD_CASES]
    for c, p in zip(cases + L.DGRAD_CASES, _run(driver, lines)):
        assert p["kernel"] != "UNSUPPORTED", c.name
        if c.pref != "AUTO":
            assert p["kernel"] == c.pref, (c.name, p["kernel"])
        if getattr(c, "wfrag", 0):
            assert (p["kernel"], p["mode"]) == ("ROWBAND", c.wfrag), (c.name, p)
        if c.ws:
            assert p["need"] > 0 and p["ksplit"] > 1 and p["ws"] == p["need"], (c.name, p)
        if getattr(c, "pool", False) and c.pref != "IGEMM4_128":
            assert p["pool"] == 1, (c.name, p)
