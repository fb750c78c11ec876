"""GPU: BFV / BGV slot encode and decode (ntt_plan_enable_slots, ntt_slots_encode_batch, ntt_slots_decode_batch / _strided).  Every
output word against the model of tests/slots_model.py, bit for bit: the device tables; the fused route over sizes, batches, the
persistent loop's wrap and every built instance; the composition at the sizes and policies the fused kernels do not serve; fused ==
composition; corner words; padded layouts among canaries; the rotation, row-swap and product statements through the shipped Galois and
product calls; a round trip through the RNS; argument errors that write nothing; the plain-C example; and two kernel traces."""
import ctypes as C
import os

import numpy as np
import pytest

import children
import galois_model as gm
import rns_support as rs
import slots_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PY = os.path.join(ROOT, "tests", "slots_model.py")
T17 = 65537
DIRS = ["encode", "decode"]


# ---------------------------------------------------------------- tables

@pytest.mark.gpu
@pytest.mark.parametrize("logn", [1, 6, 14, 15])
def test_device_tables_match_the_model(lib, logn):
    n = 1 << logn
    p = sm.plan_for(lib, n, T17)
    p.enable_slots()  # idempotent
    pos, ipos = p.slot_table(), p.slot_table(inverse=True)
    p.destroy()
    assert np.array_equal(pos, sm.pos_table(n))
    assert np.array_equal(ipos, sm.ipos_table(n))
    for i in {0, 1, n // 2 - 1, n // 2, n - 1}:
        assert lib.slot_position(n, i) == int(pos[i])
    assert lib.slot_position(n, n) is None and lib.slot_position(3 * n, 0) is None


@pytest.mark.gpu
def test_tables_and_option_before_and_after_enabling(lib):
    n = 1 << 8
    p = lib.Plan(n, T17, lib.min_root(T17, n))
    with pytest.raises(lib.NttError):
        p.slot_table()
    assert p.get_option(lib.OPT_SLOTS_FUSED) == -1
    for v, want in ((1, 1), (0, 0), (7, 1), (-1, -1)):
        p.set_option(lib.OPT_SLOTS_FUSED, v)
        assert p.get_option(lib.OPT_SLOTS_FUSED) == want
    p.enable_slots()
    assert p.slot_table().size == n
    p.destroy()


# ---------------------------------------------------------------- the fused route

@pytest.mark.gpu
@pytest.mark.parametrize("logn", [6, 12, 13, 14])
@pytest.mark.parametrize("batch", [1, 3, 130])
@pytest.mark.parametrize("direction", DIRS)
def test_fused_route(lib, oracle, logn, batch, direction):
    """2^6: the smallest instance (64 sub-blocks per workgroup); 2^13: two blocks per workgroup, an odd batch idles one half"""
    sm.run_case(lib, oracle, 1 << logn, T17, batch, direction, fused=1, seed=logn + batch)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,grid,batch", [(6, 3, 7), (12, 3, 7), (13, 3, 7), (14, 3, 7), (6, 1, 130), (13, 1, 5)])
@pytest.mark.parametrize("direction", DIRS)
def test_persistent_loop_wrap(lib, oracle, logn, grid, batch, direction):
    """NTT_OPT_MAX_GRID 3 and batch 7: the loop wraps from 2^12 on (2^13 decode: 2 blocks per workgroup, 6 per sweep).  At 2^6 one
    workgroup holds 64 polynomials: the grid of 1 over 130 wraps there, and a grid of 1 over 5 wraps both 2^13 kernels"""
    sm.run_case(lib, oracle, 1 << logn, T17, batch, direction, fused=1, max_grid=grid, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("pol,k,logn", rs.fused_launch_cases(), ids=["%s-k%d-logn%d" % c for c in rs.fused_launch_cases()])
def test_every_fused_instance(lib, oracle, pol, k, logn):
    """slots_inv_kernel and slots_fwd_kernel<policy, LOGN, class> through moduli of 30, 50, 51 and 52 bits"""
    sm.run_instance(lib, oracle, pol, k, logn)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("direction", DIRS)
def test_coarser_class_by_option(lib, oracle, cls, direction):
    """t = 65537 lands in class 18; NTT_OPT_F64_CLASS forces the kernels of the classes 0 and 1 onto the same words"""
    sm.run_case(lib, oracle, 1 << 10, T17, 3, direction, fused=1, f64_class=cls, seed=cls)


# ---------------------------------------------------------------- the composition

@pytest.mark.gpu
@pytest.mark.parametrize("logn", [1, 2, 5, 12, 15])
@pytest.mark.parametrize("direction", DIRS)
def test_composition(lib, oracle, logn, direction):
    sm.run_case(lib, oracle, 1 << logn, T17, 3, direction, fused=0, seed=logn)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", DIRS)
def test_sizes_without_a_fused_kernel_compose_even_when_forced(lib, oracle, direction):
    sm.run_case(lib, oracle, 1 << 5, T17, 3, direction, fused=1, seed=1)
    sm.run_case(lib, oracle, 1 << 15, T17, 2, direction, fused=1, seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("fused", [None, 1])
def test_integer_policy_plan_with_a_60_bit_modulus(lib, oracle, direction, fused):
    n = 1 << 8
    t = lib.find_prime(60, n)
    sm.run_case(lib, oracle, n, t, 3, direction, fused=fused, arith=lib.ARITH_U64, seed=60)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [6, 12, 13, 14])
@pytest.mark.parametrize("direction", DIRS)
def test_fused_equals_composition_and_the_default(lib, oracle, logn, direction):
    n = 1 << logn
    outs = [sm.run_case(lib, oracle, n, T17, 5, direction, fused=f, seed=3) for f in (1, 0, None)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.gpu
@pytest.mark.parametrize("max_grid", [0, 3])
@pytest.mark.parametrize("direction", DIRS)
def test_composition_max_grid(lib, oracle, max_grid, direction):
    sm.run_case(lib, oracle, 1 << 10, T17, 9, direction, fused=0, max_grid=max_grid, seed=9)


# ---------------------------------------------------------------- corner words, layouts

@pytest.mark.gpu
@pytest.mark.parametrize("bits", [17, 50, 52, 60])
@pytest.mark.parametrize("direction", DIRS)
def test_corner_words_and_the_all_t_minus_1_vector(lib, oracle, bits, direction):
    """0, 1, t - 1, (t - 1) / 2, (t + 1) / 2 lead every polynomial of every case (slots_model.words); here also every word t - 1"""
    n = 1 << 9
    t = T17 if bits == 17 else lib.find_prime(bits, n)
    w = sm.words(oracle, n, t, 1, 0)
    assert w[:5].tolist() == [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2]
    for fused in (1, 0):
        sm.run_case(lib, oracle, n, t, 2, direction, fused=fused, seed=bits)
        sm.run_case(lib, oracle, n, t, 2, direction, fused=fused, extreme=True)


@pytest.mark.gpu
@pytest.mark.parametrize("v_pad,a_pad", [(24, 0), (0, 8), (24, 56)])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("direction", DIRS)
def test_padded_layouts_among_canaries(lib, oracle, v_pad, a_pad, fused, direction):
    for logn in (7, 12):
        sm.run_case(lib, oracle, 1 << logn, T17, 3, direction, fused=fused, v_pad=v_pad, a_pad=a_pad, seed=v_pad + a_pad)


# ---------------------------------------------------------------- semantics through the existing calls

def _pipeline(lib, plan, v, n, batch, middle):
    """decode(middle(encode(v))): middle(dst, src) works on device pointers of [batch][N] coefficients"""
    dv, da, db, dout = (lib.DeviceBuffer(batch * n) for _ in range(4))
    dv.upload(v)
    lib.slots_encode(plan, da.ptr, dv.ptr, batch)
    middle(db.ptr, da.ptr)
    lib.slots_decode(plan, dout.ptr, db.ptr, batch)
    got = dout.download()
    assert np.array_equal(dv.download(), v)
    for b in (dv, da, db, dout):
        b.free()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("logn,fused", [(3, None), (10, 1), (10, 0), (15, None)])
@pytest.mark.parametrize("domain", ["coefficients", "ntt"])
def test_galois_maps_rotate_and_swap_the_rows(lib, oracle, logn, fused, domain):
    n, batch = 1 << logn, 2
    plan = sm.plan_for(lib, n, T17, fused=fused)
    v = sm.words(oracle, n, T17, batch, logn)

    def sigma(g):
        def middle(dst, src):
            if domain == "coefficients":
                plan.galois(dst, src, g, batch)
            else:
                plan.fwd(src, batch)
                plan.galois(dst, src, g, batch, lib.GALOIS_TRANSFORMED)
                plan.inv(dst, batch)
        return middle

    for r in (1, 3, -1):
        g = lib.galois_rotation(n, r)
        assert g == gm.rotation(n, r)
        assert np.array_equal(_pipeline(lib, plan, v, n, batch, sigma(g)), sm.rotate_rows(v, n, r)), r
    assert np.array_equal(_pipeline(lib, plan, v, n, batch, sigma(2 * n - 1)), sm.swap_rows(v, n))
    plan.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("logn,fused", [(6, 1), (12, 1), (12, 0), (15, None)])
def test_products_of_polynomials_are_slot_wise(lib, oracle, logn, fused):
    n, batch = 1 << logn, 2
    plan = sm.plan_for(lib, n, T17, fused=fused)
    v1, v2 = sm.words(oracle, n, T17, batch, 1), sm.words(oracle, n, T17, batch, 2)
    d2, a2 = lib.DeviceBuffer(batch * n).upload(v2), lib.DeviceBuffer(batch * n)
    lib.slots_encode(plan, a2.ptr, d2.ptr, batch)
    got = _pipeline(lib, plan, v1, n, batch, lambda dst, src: plan.negacyclic_mul(dst, src, a2.ptr, batch))
    assert np.array_equal(got, oracle.pointwise(v1, v2, T17))
    d2.free(), a2.free()
    plan.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
def test_round_trip_through_the_rns(lib, oracle, fused):
    """the example's pipeline at 2^8 with three primes: encode x 2, centred lifts, product and rotation in the NTT domain, out of the
    RNS (BGV form), decode.  |coefficients of the product| <= N (t / 2)^2 < 2^39, far inside Q / 2"""
    n, batch, steps = 1 << 8, 2, 3
    primes, roots = rs.chain(lib, n, [50, 50, 50])
    plans = [lib.Plan(n, q, w) for q, w in zip(primes, roots)]
    pt = sm.plan_for(lib, n, T17, fused=fused)
    v1, v2 = sm.words(oracle, n, T17, batch, 11), sm.words(oracle, n, T17, batch, 12)
    L, w = len(primes), batch * n
    dv = [lib.DeviceBuffer(w).upload(v) for v in (v1, v2)]
    dm = [lib.DeviceBuffer(w) for _ in range(2)]
    da = [lib.DeviceBuffer(L * w) for _ in range(2)]
    dc, dr, dout, dres = lib.DeviceBuffer(L * w), lib.DeviceBuffer(L * w), lib.DeviceBuffer(w), lib.DeviceBuffer(w)
    for k in range(2):
        lib.slots_encode(pt, dm[k].ptr, dv[k].ptr, batch)
        lib.rns_from_plain(plans, da[k].ptr, dm[k].ptr, T17, batch, lib.LIFT_TRANSFORMED)
    lib.rns_lincomb(plans, dc.ptr, [da[0].ptr], dms=[da[1].ptr], batch=batch)
    lib.rns_galois(plans, dr.ptr, dc.ptr, lib.galois_rotation(n, steps), batch, lib.GALOIS_TRANSFORMED)
    lib.rns_inv(plans, dr.ptr, batch)
    lib.rns_to_plain(plans, dout.ptr, dr.ptr, T17, batch)
    lib.slots_decode(pt, dres.ptr, dout.ptr, batch)
    got = dres.download()
    assert np.array_equal(got, sm.rotate_rows(oracle.pointwise(v1, v2, T17), n, steps))
    for b in dv + dm + da + [dc, dr, dout, dres]:
        b.free()
    for p in plans + [pt]:
        p.destroy()


# ---------------------------------------------------------------- argument errors

def _one_sided_plan(lib, oracle, n, t, inverse):
    """a plan built from ONE caller table: forward only, or inverse only"""
    cx = oracle.ctx(n, t, oracle.min_root(t, n))
    tab = np.ascontiguousarray(cx.table("winv" if inverse else "w"))
    h = C.c_void_p()
    u64p = C.POINTER(C.c_uint64)
    ptr = tab.ctypes.data_as(u64p)
    rc = lib._lib.ntt_plan_create_from_tables(C.byref(h), 0, n, t, None if inverse else ptr, ptr if inverse else None, lib.ARITH_AUTO)
    assert rc == 0, lib.last_error()
    p = lib.Plan.__new__(lib.Plan)
    p.h, p.N, p.q, p.root, p.device = h.value, n, t, 0, 0
    return p.enable_slots()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
def test_argument_errors_write_nothing(lib, oracle, fused):
    n, batch = 1 << 10, 2
    plan = sm.plan_for(lib, n, T17, fused=fused)
    bare = lib.Plan(n, T17, lib.min_root(T17, n))
    fwd_only, inv_only = _one_sided_plan(lib, oracle, n, T17, False), _one_sided_plan(lib, oracle, n, T17, True)
    img = oracle.fill_uniform(4 * batch * n, T17, 5)
    buf = lib.DeviceBuffer(img.size).upload(img)
    x, y = buf.ptr, buf.ptr + 8 * 2 * batch * n
    enc, dec = lib.slots_encode, lib.slots_decode
    bad = [
        ("encode: no slot tables", enc, bare, x, y, 0, None),
        ("decode: no slot tables", dec, bare, x, y, 0, None),
        ("encode: no inverse table", enc, fwd_only, x, y, 0, None),
        ("decode: no forward table", dec, inv_only, x, y, 0, None),
        ("encode: null output", enc, plan, None, y, 0, None),
        ("encode: null input", enc, plan, x, None, 0, None),
        ("decode: null output", dec, plan, None, y, 0, None),
        ("decode: null input", dec, plan, x, None, 0, None),
        ("encode: slot stride below N", enc, plan, x, y, 0, (n - 1, n)),
        ("encode: coefficient stride below N", enc, plan, x, y, 0, (n, n - 1)),
        ("decode: slot stride below N", dec, plan, x, y, 0, (n - 1, n)),
        ("decode: coefficient stride below N", dec, plan, x, y, 0, (n, n - 1)),
        ("encode: in place", enc, plan, x, x, 0, None),
        ("decode: in place", dec, plan, x, x, 0, None),
        ("encode: the input's first word is the output's last", enc, plan, x, x + 8 * (batch * n - 1), 0, None),
        ("decode: the spans overlap under the strides", dec, plan, x, x + 8 * n, 0, (2 * n, 2 * n)),
        ("encode: a flag", enc, plan, x, y, 1, None),
        ("decode: a flag", dec, plan, x, y, 4, None),
    ]
    for what, fn, p, first, second, flags, lay in bad:
        with pytest.raises(lib.NttError):
            fn(p, first, second, batch, flags, layout=lay)
        assert np.array_equal(buf.download(), img), what
    # batch 0 is fine, with null pointers too, and writes nothing; the one-sided plans serve their own direction
    enc(plan, None, None, 0), dec(plan, None, None, 0)
    assert np.array_equal(buf.download(), img)
    dec(fwd_only, x, y, batch), enc(inv_only, x, y, batch)
    for p in (plan, bare, fwd_only, inv_only):
        p.destroy()
    buf.free()


# ---------------------------------------------------------------- the example

@pytest.mark.gpu
def test_example_lines_match_the_model(lib, oracle):
    out = children.run_example(lib, "rns_slots")
    assert out.splitlines() == sm.example_model(lib, oracle)


# ---------------------------------------------------------------- kernel traces

@pytest.mark.gpu
def test_route_proof_one_launch_per_call():
    """fused encode + decode at 2^14 x 4: exactly one slots_inv_kernel and one slots_fwd_kernel (t = 65537: class 18), nothing else"""
    launched = [k for k in children.traced(MODEL_PY, ["--route"], 300) if k.split("<")[0] not in sm.SETUP_KERNELS]
    assert launched == ["slots_inv_kernel<ArithF64,14,18>", "slots_fwd_kernel<ArithF64,14,18>"], launched


@pytest.mark.gpu
def test_launch_proof_every_new_kernel():
    launched = set(children.traced(MODEL_PY, [], 600))
    want = sm.kernel_names()
    assert len(want) == 74
    assert not sorted(want - launched), "kernels never launched: %s" % sorted(want - launched)
