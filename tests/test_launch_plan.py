"""CPU tests of the launch plan of a batched solve (csrc/cmpc_plan.h) through cmpc_plan_dump, a
plain C++ program over that header alone: which size class runs on which stream, in which order and
with which grid. The expectations were read off launch_solve as it stood at commit b4180ef (every
knob at its default), one line per launch or wait in issue order; they are not output of the code
under test."""
import importlib
import subprocess

import pytest

K_HDR, K_HDR_CALL, K_HDR_BATCH = 32, 30, 31


@pytest.fixture(scope="module")
def dump():
    exe = importlib.import_module("quad-periodic-mpc_amd.build").build_plan_dump()

    def run(*args):
        return subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True).stdout.splitlines()
    return run


def hint_ints(batch, call=0, **counts):
    """A solve's header as the classify pass leaves it: cnt[1 + list] the list lengths."""
    h = [0] * K_HDR
    h[K_HDR_BATCH], h[K_HDR_CALL] = batch, call
    for name, count in counts.items():
        h[1 + int(name[4:])] = count
    return h


# the lines of cmpc_plan_dump
def classify(stream, c1_max, c1_listed, tail, due=0):
    return (f"classify stream={stream} fork={int(stream == 'side0')} due={due} c1_max={c1_max} "
            f"c1_listed={c1_listed} tail={tail}")


def waits(*sides):
    return [f"wait side{s} classified" for s in sides]


def tail(stream, grid, rest=0, wait="none"):
    return [f"tail stream={stream} wait={wait} list=9 grid={grid} rest={rest}",
            f"handoff stream={stream} list=10 width=80 form=persistent grid=1"]


def build64(grid):
    return f"c1_build64 stream=side1 width=64 list=7 grid={grid}"


WIDE_LIST = {80: 0, 96: 1, 120: 8, 128: 2, 144: 6, 192: 3, 256: 4}


def wide(width, side, form, grid, rest=0):
    return (f"wide w{width} stream=side{side} list={WIDE_LIST[width]} form={form} grid={grid} rest={rest} "
            f"rest_base={grid if rest else 0}")


def class1(width, over, grid, wait="none"):
    return f"class1 stream=handle wait={wait} width={width} over={over} grid={grid}"


ONE, PERSIST = "one_per_entry", "persistent"


def n10_small(batch, classify_stream, waiting, due=0):
    """N = 10 below the 60 / 64 split: one 64-wide class-1 launch, every wide class one-per-entry."""
    return (["sides 3", classify(classify_stream, 64, due, 1, due), *waits(*waiting), *tail("side2", batch),
             wide(80, 0, ONE, batch), wide(96, 1, ONE, batch), wide(120, 1, ONE, batch),
             class1(64, "list5" if due else "batch", batch), "joins 3"])


CASES = {
    "n5": ((5, 0, 1000, 0), ["sides 0", "classify none", class1(60, "batch", 1000), "joins 0"]),
    "n5_due": ((5, 0, 1000, 1), ["sides 0", classify("handle", 60, 1, 0, due=1), class1(60, "list5", 1000),
                                 "joins 0"]),
    "n10_4096": ((10, 0, 4096, 0), n10_small(4096, "side0", (1, 2))),
    "n10_8192": ((10, 0, 8192, 0), n10_small(8192, "handle", (0, 1, 2))),
    "n10_16384": ((10, 0, 16384, 0),
                  ["sides 3", classify("side0", 60, 0, 1), *waits(1, 2), *tail("side2", 16384), build64(16384),
                   wide(80, 0, ONE, 16384), wide(96, 1, PERSIST, 16384), wide(120, 1, PERSIST, 16384),
                   class1(60, "batch", 16384), "joins 3"]),
    "n10_32768_hinted": ((10, 0, 32768, 0, *hint_ints(32768, list0=2000, list1=100, list8=0, list9=3000)),
                         ["sides 3", classify("side0", 60, 0, 1), *waits(1, 2), *tail("side2", 3814, rest=32),
                          build64(32768), wide(80, 0, ONE, 2564, rest=32), wide(96, 1, PERSIST, 189),
                          wide(120, 1, PERSIST, 64), class1(60, "batch", 32768), "joins 3"]),
    "n10_131072": ((10, 0, 131072, 0),
                   ["sides 2", classify("side0", 60, 0, 1), *waits(1), build64(131072), wide(80, 0, ONE, 131072),
                    wide(96, 1, PERSIST, 131072), wide(120, 1, PERSIST, 131072), class1(60, "batch", 131072),
                    *tail("handle", 131072, wait="classified"), "joins 2"]),
    "n16_refine_4096": ((16, 1, 4096, 0),
                        ["sides 2", classify("side0", 64, 1, 0), *waits(1), wide(80, 0, ONE, 4096),
                         wide(96, 1, ONE, 4096), wide(120, 0, ONE, 4096), wide(128, 1, ONE, 4096),
                         wide(144, 0, PERSIST, 4096), wide(192, 1, PERSIST, 4096),
                         class1(64, "list5", 4096, wait="classified"), "joins 2"]),
    "n20_refine_16384": ((20, 1, 16384, 0),
                         ["sides 2", classify("side0", 60, 1, 0), *waits(1), build64(16384),
                          wide(80, 0, PERSIST, 16384), wide(96, 1, PERSIST, 16384), wide(120, 0, ONE, 16384),
                          wide(128, 1, ONE, 16384), wide(144, 0, PERSIST, 16384), wide(192, 1, PERSIST, 16384),
                          wide(256, 0, PERSIST, 16384), class1(60, "list5", 16384, wait="classified"), "joins 2"]),
    "n10_due_4096": ((10, 0, 4096, 1), n10_small(4096, "handle", (0, 1, 2), due=1)),
    # a due solve scales a due solve's counts by the whole batches: 16384 / 8192, then x 1.25 + 64
    "n10_due_hinted": ((10, 0, 16384, 1, *hint_ints(2048, call=8192, list0=1000, list1=40, list8=0, list9=600)),
                       ["sides 3", classify("handle", 60, 1, 1, due=1), *waits(0, 1, 2),
                        *tail("side2", 1564, rest=32), build64(16384), wide(80, 0, ONE, 2564, rest=32),
                        wide(96, 1, PERSIST, 164), wide(120, 1, PERSIST, 64), class1(60, "list5", 16384),
                        "joins 3"]),
    # an unmasked solve after that due solve: by the instances the due solve counted (16384 / 2048)
    "n10_hinted_by_due": ((10, 0, 16384, 0, *hint_ints(2048, call=8192, list0=1000, list1=40, list8=0, list9=600)),
                          ["sides 3", classify("side0", 60, 0, 1), *waits(1, 2), *tail("side2", 6064, rest=32),
                           build64(16384), wide(80, 0, ONE, 10064, rest=32), wide(96, 1, PERSIST, 464),
                           wide(120, 1, PERSIST, 64), class1(60, "batch", 16384), "joins 3"]),
    # below 16384 instances a hint is not used; a hint of an empty header (no solve yet) neither
    "n10_4096_hint_unused": ((10, 0, 4096, 0, *hint_ints(4096, list0=10, list9=10)),
                             n10_small(4096, "side0", (1, 2))),
    "n10_16384_hint_empty": ((10, 0, 16384, 0, *hint_ints(0)),
                             ["sides 3", classify("side0", 60, 0, 1), *waits(1, 2), *tail("side2", 16384),
                              build64(16384), wide(80, 0, ONE, 16384), wide(96, 1, PERSIST, 16384),
                              wide(120, 1, PERSIST, 16384), class1(60, "batch", 16384), "joins 3"]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_plan(dump, case):
    args, expected = CASES[case]
    assert dump(*args) == expected


def parent_chain(n, c1_max, c1_listed, tail):
    """The classify pass's ternary chain as it stood at commit b4180ef, literally."""
    return ((5 if c1_listed else -1) if n <= c1_max else 7 if n <= 64
            else (9 if (tail and n <= 72) else 0) if n <= 80
            else 1 if n <= 96 else 8 if n <= 120
            else 2 if n <= 128 else 6 if n <= 144 else 3 if n <= 192 else 4)


def test_size_class_sweep(dump):
    rows = iter(dump("classes", 240))
    for c1_max in (60, 64):
        for c1_listed in (0, 1):
            for tail_on in (0, 1):
                head, _, body = next(rows).partition(":")
                assert head == f"c1_max={c1_max} c1_listed={c1_listed} tail={tail_on}"
                assert [int(x) for x in body.split()] == [parent_chain(n, c1_max, c1_listed, tail_on)
                                                          for n in range(241)]
    assert next(rows, None) is None


# ---- the builds of the wide kernel template (csrc/cmpc_wide_builds.h) and the choice among them
def build_line(width, form, refine, literal):
    return f"w{width} form={form} refine={refine} literal={literal}"


def test_wide_build_table(dump):
    """The 21 builds, as the 21 cmpc_wide_w*.hip units of commit ec0c88f stood: 80 both forms x both
    refine values; 96 and 120 those four and the two refining forms with the literal model; 128
    refining, both forms; 144, 192 and 256 refining, persistent only."""
    expected = [build_line(80, f, r, 0) for r in (0, 1) for f in (ONE, PERSIST)]
    for width in (96, 120):
        expected += [build_line(width, f, r, 0) for r in (0, 1) for f in (ONE, PERSIST)]
        expected += [build_line(width, f, 1, 1) for f in (ONE, PERSIST)]
    expected += [build_line(128, f, 1, 0) for f in (ONE, PERSIST)]
    expected += [build_line(width, PERSIST, 1, 0) for width in (144, 192, 256)]
    assert len(expected) == 21
    got = dump("builds")
    assert len(got) == len(set(got)) == 21
    assert sorted(got) == sorted(expected)


def parent_launcher(width, persistent, refine, mdl_default):
    """The build that the if-chains of the units cmpc_wide_w{80,96,120,128,144,192,256}.hip at commit
    ec0c88f forwarded to (persistent: deq != nullptr), literally, as (form, refine, literal)."""
    if width == 80:            # launch_wide_w80: _persist_r / _r on P.refine, else _persist / its own
        return (PERSIST if persistent else ONE, refine, 0)
    if width in (96, 120):     # the same chain, _lit on P.mdl_default under P.refine
        return (PERSIST if persistent else ONE, refine, 1 if (refine and mdl_default) else 0)
    if width == 128:           # launch_wide_w128: _persist on deq, else its own; both built refining
        return (PERSIST if persistent else ONE, 1, 0)
    return (PERSIST, 1, 0)     # 144, 192, 256: one unit each, persistent only, refining


def test_wide_build_selection(dump):
    expected = []
    for width in (80, 96, 120, 128, 144, 192, 256):
        for persistent in (0, 1):
            for refine in (0, 1):
                for mdl_default in (0, 1):
                    expected.append(f"w{width} want={PERSIST if persistent else ONE} refine={refine} "
                                    f"mdl_default={mdl_default} -> "
                                    + build_line(width, *parent_launcher(width, persistent, refine, mdl_default)))
    assert len(expected) == 56
    assert dump("select") == expected
