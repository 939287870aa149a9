#!/usr/bin/env python3
"""Record which kernel, prefetch period and state size pe_create gives a sweep of
geometries: tests/golden/plan_parent.json, the fixture of tests/test_plan_host.py.

Needs a gfx950 device.  It uses PlantOSBatch's accessors only, so it runs at any
revision that has them; the committed fixture was recorded at 7aa430b, the parent of
the commit that moved kernel selection into csrc/pe_plan.hpp.

  python tools/gen_golden_plan.py            # the sweep, with the product library
  PLANTOS_HIP_LIB=<a -DPE_DEBUG_KNOBS build> python tools/gen_golden_plan.py --knobs
                                             # adds the knob rows to the same file
  ... --out PATH                             # read and write PATH instead

One process; the handles are created and closed one after another.  The sweep moves
one axis at a time around the geometries of tests/rules_util.CFG and crosses every
threshold of the selection ladder (see cases()).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "plan_parent.json")
sys.path[:0] = [os.path.join(REPO, "rl-env_amd"), os.path.join(REPO, "tests"), REPO]

# tests/rules_util.CFG (copied: that module imports the oracle, which this tool does not need)
CFG = {
    "g20": (20, 10, 12, 6, 16), "g64": (64, 100, 120, 6, 64), "g7": (7, 3, 3, 3, 12), "g32": (32, 20, 30, 9, 24),
    "g21": (21, 8, 50, 2, 10), "g25": (25, 10, 12, 6, 16), "g15": (15, 6, 8, 4, 16), "g12r2": (12, 4, 6, 2, 10),
    "g64r32": (64, 100, 120, 32, 64), "g30r2": (30, 12, 40, 2, 10), "g16c40": (16, 6, 8, 5, 40),
    "g40c48": (40, 100, 120, 8, 48), "g25r4": (25, 10, 12, 4, 16), "g8r12": (8, 3, 3, 12, 16),
    "g8r20": (8, 3, 3, 20, 16), "g24c100": (24, 10, 12, 8, 100),
}
KNOBS = ({"PE_STEP_KERNEL": "lane"}, {"PE_STEP_KERNEL": "wave"}, {"PE_QUAD_EPB": "16"}, {"PE_QUAD_EPB": "32"},
         {"PE_TILE_CODES": "1"}, {"PE_STAGGER": "0"}, {"PE_STAGGER": "8"})
KNOB_VARS = ("PE_STEP_KERNEL", "PE_QUAD_EPB", "PE_TILE_CODES", "PE_STAGGER", "PE_LDS_FLOOR")


def case(geom, n=133, codes=0, autoreset=1, algo="original", coop=-1, every=-1, max_steps=1000, knobs=None):
    G, P, O, R, C = geom
    return dict(grid_size=G, num_plants=P, num_obstacles=O, lidar_range=R, lidar_channels=C, n=n, obs_codes=codes,
                autoreset=autoreset, map_generation_algo=algo, coop_max_done=coop, prefetch_every=every,
                max_steps=max_steps, knobs=knobs or {})


def cases():
    out = []
    # every named geometry: obs_codes 0/1 (the ones it rejects too), autoreset 0
    for g in CFG.values():
        out += [case(g), case(g, codes=1), case(g, autoreset=0)]
    # G: visit-row words (20/21), row words 1 -> 2 at R = 2 (28/29), 4 (24/25), 6 (20/21), 3 (26/27),
    # 9 (14/15)
    for R, C, Gs in ((6, 16, (19, 20, 21, 22)), (2, 10, (20, 21, 28, 29)), (4, 16, (20, 21, 24, 25)),
                     (3, 12, (20, 21, 26, 27)), (9, 24, (14, 15, 20, 21)), (6, 64, (20, 21))):
        for G in Gs:
            out += [case((G, 3, 3, R, C)), case((G, 3, 3, R, C), codes=1)]
    # C, one-word (G = 16, R = 5) and multi-word (G = 32, R = 9) rows
    for C in (3, 4, 32, 33, 64, 65, 120, 121):
        out += [case((16, 6, 8, 5, C)), case((16, 6, 8, 5, C), codes=1), case((32, 20, 30, 9, C))]
    # R
    for R in (1, 2, 14, 15):
        out += [case((16, 6, 8, R, 12)), case((16, 6, 8, R, 12), codes=1)]
    # the far kernel's geometry: 96 < G + 2R <= 128 only
    for G in (32, 33, 64):
        out += [case((G, 20, 30, 32, 64)), case((G, 20, 30, 32, 64), codes=1)]
    out.append(case(CFG["g64r32"], n=1))
    # batch size: the headline kernel's workgroup shapes
    for n in (1, 4096, 4097, 8192, 8193, 32768, 32769, 65536):
        out.append(case(CFG["g20"], n=n))
    out += [case(CFG["g20"], n=1, codes=1), case(CFG["g20"], n=65536, codes=1)]
    # the runtime kernel's byte tile by batch size and CU count
    for name in ("g32", "g7", "g8r12"):
        for n in (32768, 32769, 65536):
            out.append(case(CFG[name], n=n))
    # both map algorithms around the maze's smallest grid, and on three named geometries
    for G in (6, 7):
        for algo in ("original", "maze"):
            out.append(case((G, 2, 2, 3, 12), algo=algo))
    for name in ("g20", "g64", "g32", "g24c100"):
        out.append(case(CFG[name], algo="maze"))
    # the reset-path settings
    for name in ("g20", "g64", "g32", "g24c100", "g64r32", "g8r20"):
        for coop in (0, 5):
            out.append(case(CFG[name], coop=coop))
        for every in (0, 5):
            out.append(case(CFG[name], every=every))
        out += [case(CFG[name], coop=0, every=5), case(CFG[name], autoreset=0, every=5)]
    # the argument checks
    g20 = CFG["g20"]
    out += [case((0, 0, 0, 6, 16)), case((129, 10, 12, 6, 16)), case((20, 10, 12, 0, 16)), case((20, 10, 12, 65, 16)),
            case((20, 10, 12, 6, 0)), case((20, 10, 12, 6, 257)), case((20, 400, 12, 6, 16)), case((20, -1, 12, 6, 16)),
            case((20, 10, -1, 6, 16)), case((4, 2, 3, 2, 10)), case(g20, max_steps=0),
            case(g20, max_steps=65535), case(g20, max_steps=65536), case(g20, n=0)]
    return out


def knob_cases():
    out = []
    for k in KNOBS:
        out += [case(CFG["g20"], knobs=k), case(CFG["g20"], n=65536, knobs=k), case(CFG["g20"], codes=1, knobs=k),
                case(CFG["g64"], knobs=k), case(CFG["g32"], knobs=k), case(CFG["g32"], n=65536, knobs=k)]
    return out


def record(c):
    from plantos_amd import PlantOSBatch
    for v in KNOB_VARS:
        os.environ.pop(v, None)
    os.environ.update(c["knobs"])
    kw = {k: c[k] for k in ("grid_size", "num_plants", "num_obstacles", "lidar_range", "lidar_channels",
                            "map_generation_algo", "coop_max_done", "prefetch_every", "max_steps")}
    try:
        b = PlantOSBatch(c["n"], device="cuda:0", obs_codes=bool(c["obs_codes"]), autoreset=bool(c["autoreset"]), **kw)
    except ValueError as e:
        msg = str(e)
        if not msg.startswith("pe_create: "):
            raise
        return dict(c, error=msg[len("pe_create: "):])
    res = dict(kernel_name=b.kernel_name, kernel_variant=b.kernel_variant, prefetch_every=b.prefetch_every,
               state_bytes=b.state_bytes)
    b.close()
    return dict(c, result=res)


def main():
    import torch
    knobs = "--knobs" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    if knobs and not os.environ.get("PLANTOS_HIP_LIB"):
        raise SystemExit("--knobs needs PLANTOS_HIP_LIB=<a library built with -DPE_DEBUG_KNOBS>")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = [record(c) for c in (knob_cases() if knobs else cases())]
    doc = {"cu_count": cu, "cases": [], "knob_cases": []}
    if os.path.exists(out):
        with open(out) as f:
            doc.update(json.load(f))
    if doc["cu_count"] != cu:
        raise SystemExit(f"{out} was recorded with {doc['cu_count']} CUs, this device has {cu}")
    doc["knob_cases" if knobs else "cases"] = rows
    with open(out, "w") as f:
        f.write("{\n\"cu_count\": %d,\n" % cu)
        for key in ("cases", "knob_cases"):
            f.write("\"%s\": [\n" % key)
            f.write(",\n".join(json.dumps(r, sort_keys=True) for r in doc[key]))
            f.write("\n]%s\n" % ("," if key == "cases" else ""))
        f.write("}\n")
    print(f"{out}: {len(doc['cases'])} cases, {len(doc['knob_cases'])} knob cases, "
          f"{sum('error' in r for r in doc['cases'] + doc['knob_cases'])} rejected, {cu} CUs")


if __name__ == "__main__":
    main()
