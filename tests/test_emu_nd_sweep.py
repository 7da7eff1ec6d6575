"""CPU tier: the float64 bar of accuracy_cases.py on the strided axes and on the request space around the kernels (nd_sweep_cases.py),
under emulation: the instance table, the seeded sweep over views, strides and plain N-D requests, and the check that every column
instance of line_kernels.def has a case.  The emulation evaluates the phase factors exactly and runs a grid of two CUs: the device tier
(test_gpu_nd_sweep.py) is the one that measures the product (profiles/nd_sweep_emu.log, profiles/nd_sweep_gpu.log)."""
import os
import re

import numpy as np
import pytest

import emu_harness as emu
import exec_contract_cases as t
import nd_sweep_cases as nd

EMU_TABLE = [c for c in nd.TABLE if c.emu]
LINE_KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webgpu-fft_amd", "csrc", "line_kernels.def")


def _run(oracle, monkeypatch, case, x, want_size, init):
    for k, v in case.emu_env.items():
        monkeypatch.setenv("MI355_EMU_" + k, v)
    desc, _ = t.desc_of(case.opts)
    route, _ = emu.route_of(desc)
    got, ran, _ = emu.run_plan(desc, x, want_size, out_init=init)
    assert ran == route
    return route, got


@pytest.mark.parametrize("case", EMU_TABLE, ids=repr)
def test_table(oracle, monkeypatch, case):
    x, _, want, keep = nd.acc.data(oracle, case)
    route, got = _run(oracle, monkeypatch, case, x, want.size, None)
    assert case.route_ok(route), f"{case.name} is planned as {route.strip()}, not {case.route}"
    nd.acc.measure(oracle, case, route, got[:want.size], want, keep)
    nd.acc.forget(case)


def test_every_column_instance_has_a_case(monkeypatch):
    """every LINE_PASS_A and LINE_COL_RAGGED entry of line_kernels.def is the column axis of some case of the table, as the product's
    planner (256 compute units, the case's own switches) plans it: a new instance without a case fails here"""
    with open(LINE_KERNELS) as f:
        entries = re.findall(r"^\s*LINE_(PASS_A|COL_RAGGED)\(\s*(\d+)\s*,", f.read(), re.M)
    assert {k for k, _ in entries} == {"PASS_A", "COL_RAGGED"}, "line_kernels.def no longer lists its column instances this way"
    routes = []
    for case in nd.TABLE:
        with monkeypatch.context() as m:
            for k, v in case.env.items():
                m.setenv("MI355FFT_" + k, v)
            routes.append(emu.plan_only(t.desc_of(case.opts)[0], 256)[0])
    for family, n in entries:
        tag = ("columns[" if family == "PASS_A" else "columns-ragged[") + f"N={n},"
        assert any(tag in r for r in routes), f"no case of nd_sweep_cases.TABLE plans a {tag}...] step"


def _sweep(oracle, monkeypatch, family, seed):
    d = nd.draw(family, seed)
    dat = nd.data(oracle, d)
    x = dat.x if not d.case.in_place else np.array(dat.x)
    route, got = _run(oracle, monkeypatch, d.case, x, dat.want.size, dat.init)
    nd.check(oracle, d, route, got, dat)


@pytest.mark.parametrize("seed", range(nd.SEEDS["V"]))
def test_sweep_views(oracle, monkeypatch, seed):
    _sweep(oracle, monkeypatch, "V", seed)


@pytest.mark.parametrize("seed", range(nd.SEEDS["S"]))
def test_sweep_strides(oracle, monkeypatch, seed):
    _sweep(oracle, monkeypatch, "S", seed)


@pytest.mark.parametrize("seed", range(nd.SEEDS["P"]))
def test_sweep_plain(oracle, monkeypatch, seed):
    _sweep(oracle, monkeypatch, "P", seed)


def test_draws_are_functions_of_their_seed():
    """a draw depends on its family and seed alone, and the families keep what the planner rejects by contract out"""
    for family, count in nd.SEEDS.items():
        for seed in range(count):
            o = nd.draw(family, seed).opts
            assert o == nd.draw(family, seed).opts
            assert nd.MIN_POINTS <= int(np.prod(o["shape"])) <= nd.MAX_POINTS and all(s in nd.DIMS for s in o["shape"])
            view, lay = o.get("ioView") or {}, o.get("layout") or {}
            assert not (o.get("inPlace") and (view or o.get("zeroPad") or "inputStrides" in lay or "outputStrides" in lay))
            assert not ((view.get("output") or {}).get("clearOutside") and "outputStrides" in lay)
