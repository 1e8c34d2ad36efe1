"""The batteries of tests/test_switches_gpu.py, runnable as a child: ``python -m tests.switch_runs BATTERY OUT.npz`` runs
one battery in the environment it was started with and writes every output, and what the library reported about the path
it took (the ``report`` entry: JSON), into OUT.npz.  The C-side ``NFS_*`` switches are ``static const`` and read once per
process, so a switched path exists only in a fresh process; the parent imports the same functions and runs them under
the default environment.  Every input is made on the host from a fixed seed, so parent and child see the same bits.

Nothing here asserts anything about a result: a battery only calls the library and records.  ``SWITCHES`` at the end is
the ledger of every ``NFS_*`` name the sources read (tests/test_switches_cpu.py holds it complete).
"""
import json
import sys

import numpy as np

# ---- conv -----------------------------------------------------------------------------------------------------------------
# one whole and one ragged shape per family of the default dispatch (tests/conv_ref.py PLAIN_LAYERS / POOLED_LAYERS):
# three kernels six-wave / threads / two K parts, single kernel at 64 and 128 channels, F(5x5) with one and two K parts
CONV_PLAIN = [(2, 12, 16, 128, 128), (2, 13, 11, 256, 192), (1, 2, 3, 256, 256), (1, 8, 8, 512, 512), (3, 9, 7, 64, 64),
              (3, 8, 12, 64, 128), (4, 64, 64, 128, 128), (2, 9, 14, 128, 256), (2, 10, 10, 512, 512)]
CONV_POOLED = [(2, 12, 16, 128, 128), (1, 8, 8, 512, 512), (3, 9, 7, 64, 64), (3, 8, 12, 64, 128)]
CONV_C3 = [(2, 13, 37), (8, 120, 130)]            # conv1_1: ragged both ways; more tiles than blocks (the walk wraps)
CONV_NO_EXACT = {(4, 64, 64, 128, 128)}           # (the one large case runs the realistic input only)


def sid(shape):
    return "x".join(str(v) for v in shape)


def exact_inputs(shape):
    """the integer data of tests/test_conv_gpu.py::_exact_layer"""
    from tests import conv_ref as R
    B, H, W, Ci, Co = shape
    return dict(x=R.int_tensor((B, H, W, Ci), 11), w=R.int_tensor((3, 3, Ci, Co), 12), bias=R.int_tensor((Co,), 13),
                gy=R.int_tensor((B, H, W, Co), 14), x_in=R.int_tensor((B, H, W, Ci), 15),
                addend=R.int_tensor((B, H, W, Ci), 16))


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def _host(t):
    return t.detach().cpu().numpy()


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def gemm_last():
    import ctypes
    from neural_flow_style_amd import _lib
    buf = (ctypes.c_longlong * 11)()
    _lib.call("nfs_gemm_last", buf)
    return dict(zip(("variant", "bm", "bn", "nbuf", "pre", "ksplit", "T", "K", "N", "Z", "trialled"), (int(v) for v in buf)))


def _fresh_ws(ops, floats=0):
    """a conv workspace of exactly the size the plan is stated for (ops grows and shares it otherwise), NaN-filled; with
    ``floats`` one of at least that many"""
    import torch
    ops._conv_ws.clear()
    if floats:
        ops.conv_workspace(torch.device("cuda", torch.cuda.current_device()), floats).fill_(float("nan"))


def _poison(ops, B, H, W, Ci, Co):
    from neural_flow_style_amd import _lib
    _fresh_ws(ops, int(_lib.lib().nfs_conv3x3_workspace_floats(B, H, W, Ci, Co)))


def conv_battery(ops):
    from neural_flow_style_amd import _lib
    from tests import conv_ref as R
    out, rep = {}, {"gemm_mode": ops.gemm_mode(), "plain": {}, "pooled": {}, "c3": {}}

    def layer(tag, shape, d, masked_from):
        """forward, plain gradient and the masked gradient + addend (from the bit cache where the layer keeps one, and
        from the float mask ``masked_from``)"""
        B, H, W, Ci, Co = shape
        X, Wt, Bias, GY, ADD = _dev(d["x"]), _dev(d["w"]), _dev(d["bias"]), _dev(d["gy"]), _dev(d["addend"])
        XIN = _dev(masked_from)
        wf, wdp = ops.conv3x3_pack(Wt, 0), ops.conv3x3_pack(Wt, 1)
        r = {"fwd": ops.conv3x3_plan(B, H, W, Ci, Co), "dgrad": ops.conv3x3_plan(B, H, W, Co, Ci),
             "words": ops.conv3x3_relu_bits_words(B, H, W, Ci, Co, False)}
        rb = ops.conv3x3_relu_bits(B, H, W, Ci, Co, False, X.device)
        if rb is not None:
            rb.fill_(float("nan"))
        _poison(ops, B, H, W, Ci, Co)
        out[tag + "_y"] = _host(ops.conv3x3_fwd(X, wf, Bias, Co, relu=True, out=_nan(B, H, W, Co), relu_bits=rb))
        r["last_fwd"] = gemm_last()
        _poison(ops, B, H, W, Ci, Co)
        out[tag + "_gx"] = _host(ops.conv3x3_dgrad(GY, wdp, Ci, out=_nan(B, H, W, Ci)))
        r["last_dgrad"] = gemm_last()
        _poison(ops, B, H, W, Ci, Co)
        out[tag + "_gxf"] = _host(ops.conv3x3_dgrad(GY, wdp, Ci, x_in=XIN, addend=ADD, out=_nan(B, H, W, Ci)))
        if rb is not None and masked_from is d["x"]:
            _poison(ops, B, H, W, Ci, Co)
            out[tag + "_gxb"] = _host(ops.conv3x3_dgrad(GY, wdp, Ci, x_in=XIN, addend=ADD, out=_nan(B, H, W, Ci),
                                                        relu_bits=rb))
        return r

    for shape in CONV_PLAIN:
        d = R.layer_inputs(shape)
        rep["plain"][sid(shape)] = layer("p_" + sid(shape), shape, d, d["x"])
        if shape not in CONV_NO_EXACT:
            e = exact_inputs(shape)
            layer("e_" + sid(shape), shape, e, e["x_in"])
    for shape in CONV_POOLED:
        B, H, W, Ci, Co = shape
        tag = "q_" + sid(shape)
        d = R.layer_inputs(shape, pooled=True)
        X, Wt, Bias, GYP, ADD = _dev(d["x"]), _dev(d["w"]), _dev(d["bias"]), _dev(d["gy"]), _dev(d["addend"])
        wf, wdp = ops.conv3x3_pack(Wt, 0), ops.conv3x3_pack(Wt, 1)
        r = {"fwd": ops.conv3x3_plan(B, H, W, Ci, Co, 1), "dgrad_bits": ops.conv3x3_plan(B, H, W, Co, Ci, 1),
             "dgrad_float": ops.conv3x3_plan(B, H, W, Co, Ci, 2), "words": ops.conv3x3_relu_bits_words(B, H, W, Ci, Co, True)}
        rb = ops.conv3x3_relu_bits(B, H, W, Ci, Co, True, X.device)
        if rb is not None:
            rb.fill_(float("nan"))
        _poison(ops, B, H, W, Ci, Co)
        y, yp = ops.conv3x3_fwd_pool(X, wf, Bias, Co, relu=True, relu_bits=rb, out=_nan(B, H, W, Co),
                                     out_pool=_nan(B, H // 2, W // 2, Co))
        out[tag + "_y"], out[tag + "_yp"] = _host(y), _host(yp)
        out[tag + "_pool_of_y"] = _host(ops.avgpool2_fwd(y))
        _poison(ops, B, H, W, Ci, Co)
        out[tag + "_y_plain"] = _host(ops.conv3x3_fwd(X, wf, Bias, Co, relu=True, out=_nan(B, H, W, Co)))
        # the unfused gradient takes B H W Co floats off the head of its workspace: one large enough that the convolution
        # behind it still runs the family the plan reports
        big = int(_lib.lib().nfs_conv3x3_workspace_floats(B, H, W, Ci, Co)) + B * H * W * Co
        _fresh_ws(ops, big)
        out[tag + "_gxf"] = _host(ops.conv3x3_dgrad_pool(GYP, y, wdp, Ci, x_in=X, addend=ADD, out=_nan(B, H, W, Ci)))
        if rb is not None:
            _fresh_ws(ops, big)
            out[tag + "_gxb"] = _host(ops.conv3x3_dgrad_pool(GYP, None, wdp, Ci, x_in=X, addend=ADD, relu_bits=rb, hw=(H, W),
                                                             out=_nan(B, H, W, Ci)))
        rep["pooled"][sid(shape)] = r
    c3_out, c3_rep = c3_battery(ops)
    out.update(c3_out)
    rep.update(c3_rep)
    return out, rep


def c3_battery(ops):
    """conv1_1 (3 <-> 64 channels) on the integer data, forward and data gradient: the last part of the conv battery, and
    a battery of its own for the switches that reach nothing else"""
    out, rep = {}, {"gemm_mode": ops.gemm_mode(), "c3": {}}
    for bhw in CONV_C3:
        B, H, W = bhw
        shape = (B, H, W, 3, 64)
        e = exact_inputs(shape)
        X, Wt, Bias, GY = _dev(e["x"]), _dev(e["w"]), _dev(e["bias"]), _dev(e["gy"])
        wf, wdp = ops.conv3x3_pack(Wt, 0), ops.conv3x3_pack(Wt, 1)
        rep["c3"][sid(bhw)] = {"fwd": ops.conv3x3_plan(B, H, W, 3, 64), "dgrad": ops.conv3x3_plan(B, H, W, 64, 3)}
        out["c_%s_y" % sid(bhw)] = _host(ops.conv3x3_fwd(X, wf, Bias, 64, relu=True, out=_nan(B, H, W, 64)))
        out["c_%s_gx" % sid(bhw)] = _host(ops.conv3x3_dgrad(GY, wdp, 3, out=_nan(B, H, W, 3)))
    return out, rep


# ---- rotate ---------------------------------------------------------------------------------------------------------------
# one voxel short of and past multiples of the 14 x 14 x 34 adjoint tile, an axis of length 1, and 3 x 4 = 12 (z, y) tile
# columns of two x tiles: more than eight, no multiple of eight, so two XCDs own nothing and the others own two columns
ROT_SHAPES = [(13, 27, 33), (15, 29, 69), (1, 20, 24), (29, 43, 35)]
ROT_VIEWS = ("uniform8", "scaled")


def rot_views(kind):
    """the views of tests/test_view_path_gpu.py, float32 on the host"""
    from neural_flow_style_amd import synthetic as S
    import neural_flow_style_amd.transform as T
    if kind == "uniform8":
        m = S.uniform_views(8)
    else:
        m = [1.4 * (T.rot_y_3d(-5.18) @ T.rot_z_3d(-37.6)), np.eye(3) * 1.4]
    return np.asarray(m, np.float32).reshape(-1, 3, 3)


def rot_inputs(shape, kind):
    """(views, g [V,D,H,W], what the accumulate form starts from, density, image gradient), host-seeded"""
    R = rot_views(kind)
    rng = np.random.RandomState(1000 + sum(shape) + len(kind))
    V = R.shape[0]
    return dict(R=R, g=rng.randn(V, *shape).astype(np.float32), init=(rng.rand(*shape) * 4 - 2).astype(np.float32),
                d=np.where(rng.rand(*shape) > 0.3, rng.rand(*shape), 0.0).astype(np.float32),
                g_img=rng.randn(V, *shape[1:]).astype(np.float32))


def rotate_battery(ops):
    import torch
    out, rep = {}, {"coef": []}
    for shape in ROT_SHAPES:
        for kind in ROT_VIEWS:
            c = rot_inputs(shape, kind)
            tag = "%s_%s" % (sid(shape), kind)
            R, g = _dev(c["R"]), _dev(c["g"])
            out[tag + "_w"] = _host(ops.rotate_bwd(g[..., None].contiguous(), R))
            acc = _dev(c["init"])[..., None].contiguous()
            ops.rotate_bwd(g[..., None].contiguous(), R, g_d_acc=acc)
            out[tag + "_acc"] = _host(acc)
            if ops.render_coef_layout(R.shape[0], *shape) is None:
                continue
            rep["coef"].append(tag)
            d = _dev(c["d"])
            img, rs, u, seg = ops.rotate_render_fwd_coef(d, R, 0.5)
            ab, bounds = ops.render_ray_coef(_dev(c["g_img"]), seg, 0.5)
            for k, t in (("u", u), ("seg", seg), ("ab", ab), ("bounds", bounds)):
                out["%s_coef_%s" % (tag, k)] = _host(t)
            out[tag + "_coef_w"] = _host(ops.rotate_bwd_coef(u, ab, R, bounds))
            acc = _dev(c["init"]).clone()
            ops.rotate_bwd_coef(u, ab, R, bounds, g_d_acc=acc)
            out[tag + "_coef_acc"] = _host(acc)
    torch.cuda.synchronize()
    return out, rep


# ---- ever -----------------------------------------------------------------------------------------------------------------
EVER_SHAPES = [(3, 5, 68), (9, 10, 92), (12, 20, 68)]


def ever_battery(ops):
    """the shapes and the three steps of tests/test_field_gpu.py::test_ever_skipping_is_bit_identical_over_three_steps,
    with the ever mask (the path NFS_EVER_LANES switches) and without it"""
    import torch
    from tests import field_ref as FR
    lr_t, adam = float(np.float32(3e-3)), (FR.B1, FR.B2, FR.ADAM_EPS)
    out = {}
    for shape in EVER_SHAPES:
        for kind in FR.KINDS:
            d, v, _ = FR.make_case(shape, 1, kind, "smoke")
            dt = _dev(d)
            for ever_on in (False, True):
                vel, m, u = _dev(v), torch.zeros(shape + (3,), device="cuda"), torch.zeros(shape + (3,), device="cuda")
                live = ops.live_mask(*shape, dt)
                ever = ops.live_mask(*shape, dt) if ever_on else None
                adv = ops.advect_fwd(dt, vel, live=live)[..., 0].contiguous()
                rs = np.random.RandomState(8)
                for step in range(3):
                    gt = _dev(rs.randn(*shape, 1).astype(np.float32))
                    ops.advect_bwd_adam(dt, vel, gt, m, u, lr_t, *adam, adv_next=adv, live_next=live, ever=ever)
                    tag = "%s_%s_%d_%d" % (sid(shape), kind, int(ever_on), step)
                    for k, t in (("vel", vel), ("m", m), ("v", u), ("adv", adv), ("live", live)):
                        out["%s_%s" % (tag, k)] = _host(t).view(np.int32).copy()
                    if ever_on:
                        out[tag + "_ever"] = _host(ever).view(np.int32).copy()
    return out, {}


# ---- gram -----------------------------------------------------------------------------------------------------------------
# (B, HW, C) of tests/loss_ref.py GRAM_SHAPES: one slab by default (many tile pairs, five chunks), several slabs with a
# pixel count that is no multiple of the 32-pixel chunk, and several slabs of whole chunks but for the last
GRAM_SHAPES = [(8, 144, 512), (3, 5003, 64), (1, 1000, 128)]
GRAM_GROUP = [(1025, 64), (600, 64), (30, 512)]


def gram_features(B, HW, C, seed):
    return (np.maximum(np.random.RandomState(seed).randn(B, HW, C), 0) * 30).astype(np.float32)


def gram_inputs(shape):
    """realistic features, their scale, a symmetric float32 style Gram of other features and a weight (the inputs of
    tests/test_loss_gpu.py::test_style_loss_fwd_is_float32_accurate), and the exact case of loss_ref.gram_case"""
    from tests import loss_ref as LR
    B, HW, C = shape
    F = gram_features(B, HW, C, 21)
    scale = float(np.float32(1.0 / (2.0 * HW * C)))
    Gs, _ = LR.gram(gram_features(1, HW, C, 22), scale)
    Gs = ((Gs + Gs.transpose(0, 2, 1)) / 2).astype(np.float32)
    rng = np.random.RandomState(23)
    D = rng.randn(B, C, C)
    D = ((D + D.transpose(0, 2, 1)) / 2 * 1e-3).astype(np.float32)        # a fixed symmetric D for gram_bwd
    return dict(F=F, scale=scale, Gs=Gs, w=float(np.float32(0.7)), D=D, exact=LR.gram_case(shape))


def gram_group_inputs(B=3):
    from tests import loss_ref as LR
    layers = []
    for l, (HW, C) in enumerate(GRAM_GROUP):
        F = gram_features(B, HW, C, 40 + l)
        s = float(np.float32(1.0 / (2.0 * HW * C)))
        Gs, _ = LR.gram(gram_features(1, HW, C, 60 + l), s)
        layers.append(dict(HW=HW, C=C, F=F, s=s, w=float(np.float32(0.5 + 0.25 * l)),
                           Gs=((Gs + Gs.transpose(0, 2, 1)) / 2).astype(np.float32)))
    return layers


def gram_battery(ops):
    import torch
    from neural_flow_style_amd import _lib
    out, rep = {}, {"ws": {}}
    for shape in GRAM_SHAPES:
        B, HW, C = shape
        c = gram_inputs(shape)
        tag = sid(shape)
        rep["ws"][tag] = int(_lib.lib().nfs_gram_workspace_floats(B, HW, C))
        F = _dev(c["F"])
        G = ops.gram_fwd(F, c["scale"], G=_nan(B, C, C))
        out[tag + "_G"] = _host(G)
        lacc = torch.zeros(B, device="cuda")
        Dm = ops.style_loss_fwd(G, _dev(c["Gs"]), c["w"], lacc, Dmat=_nan(B, C, C))
        out[tag + "_Dm"], out[tag + "_loss"] = _host(Dm), _host(lacc)
        out[tag + "_dF"] = _host(ops.gram_bwd(F, _dev(c["D"]), c["scale"], relu_mask=True))
        out[tag + "_Gx"] = _host(ops.gram_fwd(_dev(c["exact"]["F"]), c["exact"]["s"], G=_nan(B, C, C)))
    layers = gram_group_inputs()
    parts, dFs, Gs = ops.gram_style_group([_dev(y["F"]) for y in layers], [_dev(y["Gs"]) for y in layers],
                                          [y["w"] for y in layers], [True] * len(layers), want_G=True)
    torch.cuda.synchronize()
    out["group_parts"] = _host(parts)
    for l, (dF, G) in enumerate(zip(dFs, Gs)):
        out["group_%d_dF" % l], out["group_%d_G" % l] = _host(dF), _host(G)
    return out, rep


BATTERIES = {"conv": conv_battery, "c3": c3_battery, "rotate": rotate_battery, "ever": ever_battery, "gram": gram_battery}


def run(name):
    """(outputs, report) of battery ``name`` in this process's environment"""
    import neural_flow_style_amd.ops as ops
    first_mode = ops.gemm_mode()                 # before anything else touches it: what NFS_GEMM_MODE preset
    out, rep = BATTERIES[name](ops)
    rep["first_gemm_mode"] = first_mode
    return out, rep


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files if k != "report"}, json.loads(str(z["report"]))


# ---- the ledger of switches --------------------------------------------------------------------------------------------------
GPU = "tests.test_switches_gpu::"
MEASUREMENT = "measurement build only"
NO_EFFECT = "no effect on results"


def held(test):
    return ("test", test)


def unused(why):
    return (NO_EFFECT, why)


# every NFS_* name read with getenv in csrc/ or from os.environ in the package -> ("test", id of the test that sets it),
# (MEASUREMENT, where) for reads inside #ifdef NFS_ABLATE, or (NO_EFFECT, a one-line reason)
SWITCHES = {
    # conv dispatch
    "NFS_WINOGRAD_TILE": held(GPU + "test_winograd_tile_2"),
    "NFS_NO_WINOGRAD": held(GPU + "test_no_winograd"),
    "NFS_WG5": held(GPU + "test_wg5_and_fused_off"),
    "NFS_WG_FUSED": held(GPU + "test_wg5_and_fused_off"),
    "NFS_WG_FUSED_RAG": held(GPU + "test_wg_fused_rag_off"),
    "NFS_NO_POOL_FUSION": held(GPU + "test_no_pool_fusion"),
    "NFS_NO_RELU_BITS": held(GPU + "test_no_relu_bits"),
    "NFS_C3_OLD": held(GPU + "test_c3_old"),
    "NFS_C3F_BLOCKS": held(GPU + "test_c3_blocks"),
    "NFS_C3D_BLOCKS": held(GPU + "test_c3_blocks"),
    "NFS_WINOGRAD_MIN_CH": held(GPU + "test_winograd_min_ch_128"),
    "NFS_GEMM_MODE": held(GPU + "test_gemm_mode_0_from_the_environment"),
    # other library switches
    "NFS_RT_XCD": held(GPU + "test_rt_xcd"),
    "NFS_EVER_LANES": held(GPU + "test_ever_lanes_off"),
    "NFS_GRAM_CPS": held(GPU + "test_gram_cps"),
    # python side
    "NFS_FUSE_ADAM": held(GPU + "test_python_side_switch"),
    "NFS_FUSE_INPUT": held(GPU + "test_python_side_switch"),
    "NFS_GRAM_GROUP": held(GPU + "test_python_side_switch"),
    "NFS_GRAM_TOP_INLINE": held(GPU + "test_python_side_switch"),
    "NFS_NO_DEFER_MASK": held(GPU + "test_python_side_switch"),
    "NFS_RENDER_COEF": held(GPU + "test_python_side_switch"),
    "NFS_HIST_WIDE": held(GPU + "test_python_side_switch"),
    "NFS_SLAB_PACK": held(GPU + "test_slab_pack_torch_equals_the_copy_kernel"),
    # held before
    "NFS_SM_ROWS": held("tests.test_field_gpu::test_smooth3d_relu_sixteen_row_instance_in_a_child_process"),
    "NFS_SPLAT_LDS": held("tests.test_splat_gpu::test_lds_switched_off_in_a_child_process"),
    "NFS_LAP_UP": held("tests.test_lap_kernels_gpu::test_lap_up3_cell_kernel"),
    "NFS_MAXNORM_3K": held("tests.test_ops_gpu::test_maxnorm_input_one_launch_equals_three_launches"),
    "NFS_RB_NOSEG": held("tests.test_ops_gpu::test_render_bwd_segment_counts"),
    "NFS_RB_SEG": held("tests.test_ops_gpu::test_render_bwd_segment_counts"),
    "NFS_RR_NOSEG": held("tests.test_ops_gpu::test_rotate_render_march_variants_agree"),
    "NFS_RR_TILE": held("tests.test_ops_gpu::test_rotate_render_march_variants_agree"),
    "NFS_RR_BAND": held("tests.test_ops_gpu::test_rotate_render_march_variants_agree"),
    "NFS_RR_NOREUSE": held("tests.test_ops_gpu::test_rotate_render_march_variants_agree"),
    "NFS_W4_WAVES6_MAX": held("tests.test_ops_gpu::test_the_two_transform_schedules_agree_bit_for_bit_at_equal_batch"),
    "NFS_W5_WAVES7_MAX": held("tests.test_ops_gpu::test_the_two_transform_schedules_agree_bit_for_bit_at_equal_batch"),
    "NFS_RB16S_UNROLL": held("tests.test_gemm_unrolled_gpu::test_unrolled_and_rolled_k_loop_agree_bit_for_bit_and_are_float32_accurate"),
    "NFS_RB16S_PRE_ROWS": held("tests.test_ops_gpu::test_split_limb_gemm_from_limb_planes_and_from_the_float_pack_is_bit_identical"),
    "NFS_GEMM_TUNE": held("tests.test_ops_gpu::test_the_two_transform_schedules_agree_bit_for_bit_at_equal_batch"),
    "NFS_GRAPH": held("tests.test_engine_state_cpu::test_graph_from_env_reads_nfs_graph"),
    "NFS_DEAD_SKIP": held("tests.test_lapnorm_stylizer_gpu::test_dead_region_skipping_leaves_every_bit"),
    "NFS_FUSE_ADVECT": held("tests.test_lapnorm_stylizer_gpu::test_the_fused_step_is_the_composition_bit_for_bit"),
    "NFS_LAP_FUSE": held("tests.test_grid_ops_gpu::test_laplacian_pyramid_normalisation_matches_the_oracle"),
    "NFS_SLAB_SHARD": held("tests.test_engine_gpu::test_slab_sharded_field_work_reproduces_the_single_rank_trajectory"),
    # (the three below are read into attributes, which this test sets directly)
    "NFS_VIEW_GROUPS": held("tests.test_engine_gpu::test_view_groups_on_streams_match_single_batch"),
    "NFS_VGG_STREAMS": held("tests.test_engine_gpu::test_view_groups_on_streams_match_single_batch"),
    "NFS_GRAM_STREAM": held("tests.test_engine_gpu::test_view_groups_on_streams_match_single_batch"),
    "NFS_2P_AUTOGRAD": held("tests.test_styler_gpu::test_styler2p_chain_written_out_on_the_operators_equals_the_autograd_form"),
    # measurement builds
    "NFS_CONV_DBG": (MEASUREMENT, "vgg.hip, inside #ifdef NFS_ABLATE"),
    "NFS_GEMM_DBG": (MEASUREMENT, "winograd.hip, inside #ifdef NFS_ABLATE"),
    # no effect on results
    "NFS_LIB_PATH": unused("which build of the same library is loaded"),
    "NFS_VERBOSE": unused("prints the graph trial's timings"),
    "NFS_GEMM_TUNE_LOG": unused("prints the tile tuner's choice to stderr"),
    "NFS_SYNTHETIC_VGG": unused("asks for synthetic weights where no weight file is given; the tests pass weights"),
}


if __name__ == "__main__":
    battery, path = sys.argv[1], sys.argv[2]
    outputs, report = run(battery)
    np.savez(path, report=np.array(json.dumps(report)), **outputs)
    print("switch_runs %s: %d outputs, report %s" % (battery, len(outputs), json.dumps(report)[:2000]))
