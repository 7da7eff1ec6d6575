"""CPU tier: boundary "circular" on the six overlap-save routes of fftconv (route tags ending in ",wrap]") under host emulation.

The case table and its bars are fftconv_circular_cases.py's, shared with the GPU tier: float64 circular references, the same request with
OLS_CIRCULAR at 0, for real data the complex plan on the widened data, the exact route tag, 1 + K launches and K P^rank 8 bytes of workspace.
Then the strided requests, the capabilities the routes add (requests that had no plan, or a widened one), the planner alone on the rule, the
switch, the bounds and the neighbours whose plans must not move, every linear request of the existing tables under the three values of the
switch, and the exec contract (exec_contract_cases.py's harness: guard bands catch a load or store outside a block's predicates) on a dense
and a strided request per route."""
import numpy as np
import pytest

import emu_harness as emu
import fftconv_bricks_cases as bricks
import fftconv_circular_cases as circ
import fftconv_cols_cases as cols
import fftconv_ols_cases as ols
import fftconv_ols_scaffold as scaffold
import fftconv_rbricks_cases as rbricks
import fftconv_rtiles_cases as rtiles
import fftconv_tiles_cases as tiles
import test_emu_exec_contract as contract
from mi355fft import _abi
from test_emu_fftconv_real import _desc, _opts

ENV = "MI355FFT_" + circ.SWITCH       # the product planner's form of the switch: emu.plan_only reads the library's environment


@pytest.mark.parametrize("rc", circ.CASES, ids=circ.case_id)
def test_circular_overlap_save(oracle, monkeypatch, rc):
    route, case = rc
    route.check_case(*scaffold.emu_runner(monkeypatch), oracle, case)


@pytest.mark.parametrize("route", circ.ROUTES, ids=lambda r: r.tag[:-1])
def test_strided_lanes_on_both_sides(oracle, monkeypatch, route):
    def unsupported(opts):
        with pytest.raises(emu.EmuError) as e:
            emu.route_of(_desc(opts)[0])
        assert circ.UNSUPPORTED in str(e.value) and e.value.code == _abi.ERR_UNSUPPORTED
    route.check_strided(*scaffold.emu_runner(monkeypatch), oracle, unsupported)


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(route, shape, ks, batch=1, K=1, mode="convolution", boundary="circular", layout=None):
    opts = route.options(shape, ks, batch, K=K, mode=mode, boundary=boundary)
    if layout:
        opts["layout"] = dict(opts.get("layout") or {}, **layout)
    return emu.plan_only(_desc(opts)[0])


def _block(route, rule):
    return rule ** route.rank * 8


@pytest.mark.parametrize("rc", circ.CASES, ids=circ.case_id)
def test_route_launches_and_workspace(monkeypatch, rc):
    """the tag ends in ",wrap]", 1 + K launches, K P^rank 8 bytes of workspace (and the tables, which are no workspace); at 0 the tag is gone"""
    route, case = rc
    desc = _desc(case.opts)[0]
    got, launches, work = emu.plan_only(desc)
    assert case.tag in got and case.tag.endswith(",wrap]") and launches == 1 + case.K, (got, launches)
    assert not any(f in got for f in route.forbidden), got
    spectrum = (case.rule // 2 + 1) * 8 if route.real and route.rank == 1 else _block(route, case.rule)      # real lines: packed bins
    assert work == -(-case.K * spectrum // 256) * 256, (got, work)           # (the planner sizes its workspace in 256-byte units)
    monkeypatch.setenv(ENV, "0")
    assert ",wrap]" not in emu.plan_only(desc)[0]


def test_capability_a_complex_line_of_5000000_points(monkeypatch):
    """complex circular 5000000 (*) 255: two launches and one block of workspace.  With the switch at 0 this length (2^6 5^7, 13-smooth) takes 30
    per-radix stage launches and 200 MB of workspace; its neighbour 5000001 has no plan at all (a Bluestein axis beyond 2^22) and takes the route too"""
    for n in (5000000, 5000001):
        route, launches, work = _plan(circ.LINES, (n,), (255,))
        assert route.endswith("lines-conv-ols[N=2048,L=1794,wrap] ") and launches == 2 and work == 2048 * 8, (route, launches, work)
    monkeypatch.setenv(ENV, "0")
    route, launches, work = _plan(circ.LINES, (5000000,), (255,))
    assert "stages[N=5000000" in route and circ.LINES.tag not in route and launches > 20 and work >= 5000000 * 8 * 4, (route, launches, work)
    with pytest.raises(emu.EmuError) as e:
        _plan(circ.LINES, (5000001,), (255,))
    assert "Unsupported: Bluestein axis length" in str(e.value) and e.value.code == _abi.ERR_UNSUPPORTED


@pytest.mark.parametrize("route", [circ.RTILES, circ.RBRICKS], ids=lambda r: r.tag[:-1])
def test_capability_strided_real_sides(monkeypatch, route):
    """real circular 150 x 130 (*) 9 x 5 and 40 x 36 x 34 (*) 5 x 3 x 4 on strided sides: no plan with the switch at 0, the route with it at 1"""
    desc = _desc(route.strided_request()[0])[0]
    monkeypatch.setenv(ENV, "0")
    with pytest.raises(emu.EmuError) as e:
        emu.plan_only(desc)
    assert circ.UNSUPPORTED in str(e.value) and e.value.code == _abi.ERR_UNSUPPORTED
    monkeypatch.setenv(ENV, "1")
    got, launches, _ = emu.plan_only(desc)
    assert route.strided_tag() in got and launches == 1 + route.strided["K"], got


def test_capability_an_odd_real_line_is_not_widened(monkeypatch):
    got = _plan(circ.RLINES, (8193,), (31,))[0]
    assert circ.RLINES.tag_of(1024, (31,)) in got and "rconv-widened" not in got and "pad[" not in got, got
    monkeypatch.setenv(ENV, "0")
    assert "rconv-widened" in _plan(circ.RLINES, (8193,), (31,))[0]


POW2 = [   # circular requests on power-of-two domains, pinned to their routes by the existing tests: (route, shape, ks, the block value 2 gives them)
    (circ.TILES, (256, 256), (9, 9), 64), (circ.BRICKS, (64, 64, 64), (3, 3, 3), 16), (circ.LINES, (1 << 17,), (129,), 2048),
    (circ.RTILES, (256, 256), (9, 9), 64), (circ.RBRICKS, (64, 64, 64), (3, 3, 3), 16), (circ.RLINES, (1 << 17,), (129,), 1024),
]


@pytest.mark.parametrize("route,shape,ks,rule", POW2, ids=lambda v: v.tag[:-1] if hasattr(v, "tag") else None)
def test_power_of_two_domains_stay_unless_forced(monkeypatch, route, shape, ks, rule):
    default = _plan(route, shape, ks, 2)
    assert route.tag not in default[0], default
    monkeypatch.setenv(ENV, "0")
    assert _plan(route, shape, ks, 2) == default          # same route, launches and workspace
    monkeypatch.setenv(ENV, "2")
    assert route.tag_of(rule, ks) in _plan(route, shape, ks, 2)[0]


def test_real_4096_line_stays(monkeypatch):
    """real 4096 (*) 64 circular (lines-rconv[N=4096]): below the route's bounds under every value of the switch"""
    plans = []
    for v in ("0", "1", "2"):
        monkeypatch.setenv(ENV, v)
        plans.append(_plan(circ.RLINES, (4096,), (64,), 4))
    assert plans[0] == plans[1] == plans[2] and "lines-rconv[N=4096]" in plans[0][0], plans


def test_lines_above_2_22_points_move_whatever_their_length(monkeypatch):
    assert circ.LINES.tag_of(2048, (255,)) in _plan(circ.LINES, (1 << 23,), (255,))[0]
    assert circ.RLINES.tag_of(2048, (255,)) in _plan(circ.RLINES, (1 << 23,), (255,))[0]
    assert circ.LINES.tag not in _plan(circ.LINES, (1 << 22,), (255,))[0]


BOUNDS = [   # (route, the shape with one axis at 2 P - 1 (or its odd neighbour below), the same just above 2 P, kernel, P, a kernel beyond the linear route's bound)
    (circ.RLINES, (16383,), (16385,), (300,), 8192, (4097,)),
    (circ.TILES, (150, 127), (150, 129), (9, 5), 64, (34, 5)),
    (circ.RTILES, (127, 150), (129, 150), (9, 5), 64, (9, 34)),
    (circ.BRICKS, (40, 36, 31), (40, 36, 33), (3, 3, 3), 16, (10, 3, 3)),
    (circ.RBRICKS, (31, 36, 40), (33, 36, 40), (3, 3, 3), 16, (3, 10, 3)),
]


@pytest.mark.parametrize("route,below,at,ks,P,beyond", BOUNDS, ids=lambda v: v.tag[:-1] if hasattr(v, "tag") else None)
def test_the_bounds(monkeypatch, route, below, at, ks, P, beyond):
    """shape[a] = 2 P - 1 stays and 2 P goes (by default its odd neighbour 2 P + 1, under value 2 the power of two itself); a kernel beyond the
    linear route's bound stays under every value"""
    assert route.tag not in _plan(route, below, ks)[0], below
    assert route.tag_of(P, ks) in _plan(route, at, ks)[0], at
    assert route.tag not in _plan(route, at, beyond)[0], beyond
    monkeypatch.setenv(ENV, "2")
    exact = tuple(2 * P if a != b else a for a, b in zip(below, at))          # the axis that moved, at exactly 2 P
    assert route.tag_of(P, ks) in _plan(route, exact, ks)[0], exact
    assert route.tag not in _plan(route, below, ks)[0], below
    assert route.tag not in _plan(route, at, beyond)[0], beyond


def test_the_bounds_of_complex_lines(monkeypatch):
    """the floor of the route's own rule (more than 16384 points) lies above 2 P for both of its blocks, so it is the bound that binds; kernels
    beyond 513 points stay"""
    route = circ.LINES
    assert route.tag_of(4096, (513,)) in _plan(route, (16411,), (513,))[0]
    assert route.tag not in _plan(route, (16411,), (514,))[0]
    assert route.tag not in _plan(route, (16383,), (65,))[0]
    monkeypatch.setenv(ENV, "2")
    assert route.tag not in _plan(route, (16384,), (65,))[0] and route.tag_of(2048, (65,)) in _plan(route, (16385,), (65,))[0]
    assert route.tag not in _plan(route, (16411,), (514,))[0]


SWITCHES = [   # (route, request, the route's own switch, the switches in front of it)
    (circ.LINES, ((16411,), (65,)), "CONV_OLS", (("CONV_LINES", "0"), ("FORCE_GENERIC", "1"))),
    (circ.RLINES, ((8193,), (31,)), "RCONV_OLS", (("RCONV_FUSED", "0"), ("FORCE_GENERIC", "1"))),
    (circ.TILES, ((150, 130), (9, 5)), "CONV_OLS2D", (("CONV_LINES", "0"), ("FORCE_GENERIC", "1"), ("FUSE_VIEWS", "0"))),
    (circ.RTILES, ((150, 130), (9, 5)), "RCONV_OLS2D", (("RCONV_FUSED", "0"), ("FORCE_GENERIC", "1"), ("FUSE_VIEWS", "0"))),
    (circ.BRICKS, ((40, 36, 34), (3, 3, 3)), "CONV_OLS3D", (("CONV_LINES", "0"), ("FORCE_GENERIC", "1"), ("FUSE_VIEWS", "0"))),
    (circ.RBRICKS, ((40, 36, 34), (3, 3, 3)), "RCONV_OLS3D", (("RCONV_FUSED", "0"), ("FORCE_GENERIC", "1"), ("FUSE_VIEWS", "0"))),
]


@pytest.mark.parametrize("route,request_,own,front", SWITCHES, ids=lambda v: v.tag[:-1] if hasattr(v, "tag") else None)
def test_the_switches(monkeypatch, route, request_, own, front):
    """the route's own switch at 0 and the switches in front of it turn the circular form off; forced to a block it moves no circular request"""
    shape, ks = request_
    taken = _plan(route, shape, ks, 2)
    assert route.tag in taken[0]
    for name, value in ((own, "0"),) + front:
        monkeypatch.setenv("MI355FFT_" + name, value)
        assert route.tag not in _plan(route, shape, ks, 2)[0], name
        monkeypatch.delenv("MI355FFT_" + name)
    for forced in {1: ("128", "256", "4096"), 2: ("64", "128"), 3: ("16",)}[route.rank]:
        monkeypatch.setenv("MI355FFT_" + own, forced)
        assert _plan(route, shape, ks, 2) == taken, forced                     # the rule's block, not the forced one
        small = tuple(n // 4 for n in shape)                                   # inside the forced block's reach, outside the rule's
        monkeypatch.setenv(ENV, "0")
        at0 = _plan(route, small, ks, 2)
        monkeypatch.delenv(ENV)
        assert _plan(route, small, ks, 2) == at0 and route.tag not in at0[0], (forced, small)
    monkeypatch.delenv("MI355FFT_" + own)


LINEAR_TABLES = [(cols.ROUTE, cols.CASES), (ols.ROUTE, ols.CASES), (tiles.ROUTE, tiles.CASES), (rtiles.ROUTE, rtiles.CASES), (bricks.ROUTE, bricks.CASES),
                 (rbricks.ROUTE, rbricks.CASES)]


@pytest.mark.parametrize("route,cases", LINEAR_TABLES, ids=lambda v: v.tag[:-1] if hasattr(v, "tag") else None)
def test_linear_requests_plan_identically(monkeypatch, route, cases):
    """every linear request of the six routes' tables: the same route, launches and workspace with the switch at 0, 1 and 2"""
    for case in cases:
        if case.P is not None:
            monkeypatch.setenv("MI355FFT_" + route.switch, str(case.P))
        else:
            monkeypatch.delenv("MI355FFT_" + route.switch, raising=False)
        plans = []
        for v in ("0", "1", "2"):
            monkeypatch.setenv(ENV, v)
            plans.append(emu.plan_only(_desc(case.opts)[0]))
        assert plans[0] == plans[1] == plans[2] and case.tag in plans[0][0] and "wrap" not in plans[0][0], (case, plans)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", circ.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans both"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
