"""ctypes binding of libhiprec.so (declared in include/hiprec.h).

The HIP library is THE product path: there is no CPU fallback.  If the shared object is missing or
a symbol is absent, loading fails loudly with a RuntimeError naming the build command.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64
from ctypes import c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIPREC_LIB selects another build of the same sources, e.g. libhiprec_ieee.so (-DHIPREC_IEEE_DIV: ATen's
# correctly rounded sqrt / division in the Adam / RMSprop denominators, op for op)
LIB_PATH = os.path.join(_HERE, os.environ.get("HIPREC_LIB", "libhiprec.so"))

OPT_SGD, OPT_ADAM, OPT_RMSPROP = 0, 1, 2
OPT_KINDS = {"sgd": OPT_SGD, "adam": OPT_ADAM, "rmsprop": OPT_RMSPROP}
# torch.optim.RMSprop(momentum > 0), cmn.py's own optimizer: no config name of the reference selects it, so it is
# not in OPT_KINDS (HipOptimizer("rmsprop", lr, momentum=...) does)
OPT_RMSPROP_MOMENTUM = 3

STATUS_USER_OOB, STATUS_ITEM_OOB, STATUS_ROW_OOB, STATUS_ROUTE_OVERFLOW = 1, 2, 4, 8
STATUS_NEG_EXHAUSTED = 16
STATUS_LAZY_TABLE = 32
STATUS_TABLE_FULL = 64
STATUS_TIME_OOB = 128
STATUS_NOT_SPD = 256
STATUS_NOT_FINITE = 512


class MfTables(Structure):
    """hiprec_mf_tables (include/hiprec.h)."""

    _fields_ = [
        ("user_emb", c_void_p),
        ("item_emb", c_void_p),
        ("user_bias", c_void_p),
        ("item_bias", c_void_p),
        ("global_bias", c_void_p),
        ("n_users", c_int64),
        ("n_items", c_int64),
        ("dim", c_int32),
        ("_pad", c_int32),
    ]


class Stats(Structure):
    """hiprec_stats (include/hiprec.h) — host-side mirror used to decode a device copy."""

    _fields_ = [
        ("loss", c_float),
        ("reg", c_float),
        ("loss_sum", c_double),
        ("reg_sum", c_double),
        ("step", c_int64),
        ("beta1", c_double),
        ("beta2", c_double),
        ("beta1_pow", c_double),
        ("beta2_pow", c_double),
        ("status", c_uint32),
        ("_pad", c_uint32),
    ]


NCF_MAX_LAYERS = 8


class NcfPlan(Structure):
    """hiprec_ncf_plan (include/hiprec.h)."""

    _fields_ = (
        [(n, c_void_p) for n in ("user_mlp", "item_mlp", "user_mf", "item_mf",
                                 "g_user_mlp", "g_item_mlp", "g_user_mf", "g_item_mf")]
        + [("n_users", c_int64), ("n_items", c_int64),
           ("dim_mlp", c_int32), ("dim_mf", c_int32), ("n_layers", c_int32), ("relu_input", c_int32),
           ("layer_in", c_int32 * NCF_MAX_LAYERS), ("layer_out", c_int32 * NCF_MAX_LAYERS),
           ("fc_w", c_void_p * NCF_MAX_LAYERS), ("fc_b", c_void_p * NCF_MAX_LAYERS),
           ("g_fc_w", c_void_p * NCF_MAX_LAYERS), ("g_fc_b", c_void_p * NCF_MAX_LAYERS),
           ("out_w", c_void_p), ("out_b", c_void_p), ("g_out_w", c_void_p), ("g_out_b", c_void_p),
           ("max_batch", c_int64),
           ("act", c_void_p * (NCF_MAX_LAYERS + 1)), ("dact", c_void_p * (NCF_MAX_LAYERS + 1)),
           ("mf", c_void_p), ("dmf", c_void_p), ("scores", c_void_p),
           ("keep", c_void_p * NCF_MAX_LAYERS), ("keep_scale", c_float), ("_pad", c_int32)]
    )


class Csr(Structure):
    """hiprec_csr (include/hiprec.h)."""

    _fields_ = [("rowptr", c_void_p), ("col", c_void_p), ("val", c_void_p), ("eid", c_void_p),
                ("n_rows", c_int64), ("nnz", c_int64), ("slice_row", c_void_p)]


class SlicedCsr(Structure):
    """hiprec_sliced_csr (include/hiprec.h)."""

    _fields_ = [("chunks", c_void_p), ("col16", c_void_p), ("val", c_void_p), ("eid", c_void_p),
                ("sub_row", c_void_p), ("sub_chunk", c_void_p), ("spill_row", c_void_p), ("spill_ptr", c_void_p),
                ("empty_row", c_void_p), ("empty_ptr", c_void_p), ("row_scale", c_void_p), ("col_scale", c_void_p),
                ("n_rows", c_int64), ("n_slots", c_int64),
                ("n_groups", c_int32), ("subs_per_group", c_int32), ("n_chunks", c_int32), ("row_cap", c_int32),
                ("lane_slots", c_int32), ("pad_slot", c_int32)]


class LightGcnPlan(Structure):
    """hiprec_lightgcn_plan (include/hiprec.h)."""

    _fields_ = [("a", Csr), ("at", Csr), ("n_users", c_int64), ("n_items", c_int64),
                ("dim", c_int32), ("n_layers", c_int32), ("decay", c_float), ("_pad", c_int32)] + \
               [(n, c_void_p) for n in ("e0", "g", "xa", "xb", "acc", "da", "db", "zero_ws")] + \
               [("zero_ws_floats", c_int64), ("sa", SlicedCsr), ("sat", SlicedCsr), ("slice_w", c_int32),
                ("dropped_ready", c_int32), ("sliced_ws", c_void_p), ("sliced_ws_floats", c_int64)]


class PgmfTables(Structure):
    """hiprec_pgmf_tables (include/hiprec.h)."""

    _fields_ = [("user_memory", c_void_p), ("item_memory", c_void_p), ("v", c_void_p),
                ("n_users", c_int64), ("n_items", c_int64), ("dim", c_int32), ("_pad", c_int32)]


class CmnTables(Structure):
    """hiprec_cmn_tables (include/hiprec.h)."""

    _fields_ = [(n, c_void_p) for n in ("user_memory", "item_memory", "user_output", "hop_w", "hop_b", "dense_w",
                                        "dense_b", "out_w")] + \
               [("n_users", c_int64), ("n_items", c_int64), ("dim", c_int32), ("_pad", c_int32)]


class UltraGcnTables(Structure):
    """hiprec_ultragcn_tables (include/hiprec.h)."""

    _fields_ = [("user_embeds", c_void_p), ("item_embeds", c_void_p), ("n_users", c_int64), ("n_items", c_int64),
                ("dim", c_int32), ("_pad", c_int32)]


class UltraGcnParams(Structure):
    """hiprec_ultragcn_params (include/hiprec.h)."""

    _fields_ = [("beta_u", c_void_p), ("beta_i", c_void_p), ("ii_neighbor", c_void_p), ("ii_sim", c_void_p),
                ("n_neighbors", c_int32), ("w1", c_float), ("w2", c_float), ("w3", c_float), ("w4", c_float),
                ("negative_weight", c_float), ("gamma", c_float), ("lambda_", c_float)]


MIXGCF_MAX_HOPS = 6
MIXGCF_POOLS = {"concat": 0, "mean": 1, "sum": 2, "final": 3}


class MixGcfPlan(Structure):
    """hiprec_mixgcf_plan (include/hiprec.h)."""

    _fields_ = [("a", Csr), ("at", Csr), ("n_users", c_int64), ("n_items", c_int64),
                ("dim", c_int32), ("n_hops", c_int32), ("pool", c_int32), ("rns", c_int32), ("n_negs", c_int32),
                ("k_neg", c_int32), ("l2", c_float), ("edge_scale", c_float), ("mess_scale", c_float), ("_pad", c_int32),
                ("e0", c_void_p), ("g", c_void_p), ("zero_ws", c_void_p), ("zero_ws_floats", c_int64),
                ("edge_keep", c_void_p * MIXGCF_MAX_HOPS), ("mess_keep", c_void_p * MIXGCF_MAX_HOPS)]


SGL_MAX_LAYERS = 6
SGL_TILE_B = 32       # HIPREC_SGL_TILE_B / _N / MAX_SPLITS (include/hiprec.h), checked against the library at load
SGL_TILE_N = 64
SGL_MAX_SPLITS = 64


class SglPlan(Structure):
    """hiprec_sgl_plan (include/hiprec.h)."""

    _fields_ = [("a", Csr), ("at", Csr), ("s", Csr), ("sub_val", (c_void_p * SGL_MAX_LAYERS) * 2),
                ("n_users", c_int64), ("n_items", c_int64), ("dim", c_int32), ("n_layers", c_int32),
                ("ssl_sides", c_int32), ("n_splits", c_int32), ("regs", c_float), ("ssl_reg", c_float),
                ("ssl_temp", c_float), ("_pad", c_int32), ("e0", c_void_p), ("g", c_void_p), ("ws", c_void_p),
                ("ws_floats", c_int64), ("batch_ws", c_void_p), ("batch_ws_floats", c_int64)]


LCFN_MAX_LAYERS = 4
LCFN_MAX_DIM = 128     # HIPREC_LCFN_* (include/hiprec.h); the tile and slot constants are checked against the library at load
LCFN_MAX_FREQ = 256
LCFN_MAX_WIDTH = 512
LCFN_TILE_ROWS = 32
LCFN_MAX_SLOTS = 256


class LcfnPlan(Structure):
    """hiprec_lcfn_plan (include/hiprec.h)."""

    _fields_ = [("P", c_void_p), ("Q", c_void_p), ("n_users", c_int64), ("n_items", c_int64), ("f_user", c_int32),
                ("f_item", c_int32), ("dim", c_int32), ("layer", c_int32), ("train_filters", c_int32), ("n_slots", c_int32),
                ("lamda", c_float), ("_pad", c_int32), ("w", c_void_p), ("g", c_void_p), ("ws", c_void_p),
                ("ws_floats", c_int64), ("batch_ws", c_void_p), ("batch_ws_floats", c_int64)]


SIMGCL_MAX_LAYERS = 4
SIMGCL_MAX_DIM = 256   # HIPREC_SIMGCL_* (include/hiprec.h), checked against the library at load
SIMGCL_TILE_B = 32
SIMGCL_TILE_N = 64


class SimgclPlan(Structure):
    """hiprec_simgcl_plan (include/hiprec.h)."""

    _fields_ = [("a", Csr), ("at", Csr), ("n_users", c_int64), ("n_items", c_int64), ("dim", c_int32),
                ("n_layers", c_int32), ("user_view", c_int32), ("_pad", c_int32), ("eps", c_float), ("reg", c_float),
                ("lambda_", c_float), ("cl_temp", c_float), ("noise_seed", c_uint64), ("noise", c_void_p),
                ("e0", c_void_p), ("g", c_void_p), ("ws", c_void_p), ("ws_floats", c_int64), ("stamps", c_void_p),
                ("batch_ws", c_void_p), ("batch_ws_floats", c_int64)]


BUIR_MAX_LAYERS = 4
BUIR_MAX_DIM = 256     # HIPREC_BUIR_* (include/hiprec.h), checked against the library at load
BUIR_TILE_B = 32


class BuirPlan(Structure):
    """hiprec_buir_plan (include/hiprec.h)."""

    _fields_ = [("a", Csr), ("at", Csr), ("n_users", c_int64), ("n_items", c_int64), ("dim", c_int32),
                ("n_layers", c_int32), ("apply_pending", c_int32), ("_pad", c_int32), ("momentum", c_float),
                ("one_minus_momentum", c_float), ("online", c_void_p), ("target", c_void_p), ("w", c_void_p),
                ("b", c_void_p), ("g_online", c_void_p), ("g_w", c_void_p), ("g_b", c_void_p), ("ws", c_void_p),
                ("ws_floats", c_int64), ("batch_ws", c_void_p), ("batch_ws_floats", c_int64)]


class SasrecShape(Structure):
    """hiprec_sasrec_shape (include/hiprec.h)."""

    _fields_ = [("n_items", c_int64), ("dim", c_int32), ("heads", c_int32), ("maxlen", c_int32), ("n_blocks", c_int32)]


class TisasrecShape(Structure):
    """hiprec_tisasrec_shape (include/hiprec.h)."""

    _fields_ = [("n_items", c_int64), ("dim", c_int32), ("heads", c_int32), ("maxlen", c_int32),
                ("time_span", c_int32), ("n_blocks", c_int32), ("_pad", c_int32)]


class Bert4recShape(Structure):
    """hiprec_bert4rec_shape (include/hiprec.h)."""

    _fields_ = [("n_items", c_int64), ("dim", c_int32), ("heads", c_int32), ("maxlen", c_int32), ("n_blocks", c_int32),
                ("ffn_dim", c_int32), ("_pad", c_int32)]


class NarmShape(Structure):
    """hiprec_narm_shape (include/hiprec.h)."""

    _fields_ = [("n_items", c_int64), ("emb_dim", c_int32), ("hidden", c_int32), ("n_layers", c_int32), ("_pad", c_int32)]


class Gru4recShape(Structure):
    """hiprec_gru4rec_shape (include/hiprec.h)."""

    _fields_ = [("n_items", c_int64), ("n_layers", c_int32), ("hidden", c_int32 * 3), ("emb_dim", c_int32),
                ("loss", c_int32)]


class CaserShape(Structure):
    """hiprec_caser_shape (include/hiprec.h)."""

    _fields_ = [("n_users", c_int64), ("n_items", c_int64), ("dim", c_int32), ("L", c_int32), ("T", c_int32),
                ("N", c_int32), ("n_v", c_int32), ("n_h", c_int32), ("ac_conv", c_int32), ("ac_fc", c_int32)]


class SrgnnShape(Structure):
    """hiprec_srgnn_shape (include/hiprec.h)."""

    _fields_ = [("n_node", c_int64), ("hidden", c_int32), ("step", c_int32), ("nonhybrid", c_int32), ("_pad", c_int32)]


class VbcarShape(Structure):
    """hiprec_vbcar_shape (include/hiprec.h)."""

    _fields_ = [("n_users", c_int64), ("n_items", c_int64), ("emb_dim", c_int32), ("late_dim", c_int32),
                ("fea_u", c_int32), ("fea_i", c_int32), ("act", c_int32), ("_pad", c_int32)]


class TvbrShape(Structure):
    """hiprec_tvbr_shape (include/hiprec.h)."""

    _fields_ = [("n_users", c_int64), ("n_items", c_int64), ("emb_dim", c_int32), ("time_step", c_int32),
                ("fea_u", c_int32), ("fea_i", c_int32), ("act", c_int32), ("_pad", c_int32)]


class VaecfShape(Structure):
    """hiprec_vaecf_shape (include/hiprec.h)."""

    _fields_ = [("n_users", c_int64), ("n_items", c_int64), ("z_dim", c_int32), ("n_hidden", c_int32),
                ("hidden", c_int32 * 3), ("act", c_int32), ("likelihood", c_int32), ("w0_shadow", c_int32)]


class T2vTables(Structure):
    """hiprec_t2v_tables (include/hiprec.h)."""

    _fields_ = [("user_emb", c_void_p), ("item_emb1", c_void_p), ("item_emb2", c_void_p),
                ("user_bias", c_void_p), ("item_bias", c_void_p),
                ("n_users", c_int64), ("n_items", c_int64), ("dim", c_int32), ("_pad", c_int32)]


class ShardPlan(Structure):
    """hiprec_shard_plan (include/hiprec.h)."""

    _fields_ = [("world", c_int32), ("rank", c_int32), ("n_steps", c_int64), ("cap", c_int64),
                ("local_batch", c_int64), ("n_local", c_int64), ("users", c_void_p), ("pos_slot", c_void_p),
                ("neg_slot", c_void_p), ("own", c_void_p), ("total", c_void_p), ("total_stride", c_int64),
                ("in_idx", c_void_p), ("ex_req", c_void_p), ("ex_in", c_void_p), ("in_off_host", c_void_p),
                ("n_slots_host", c_void_p), ("req_cnt_host", c_void_p), ("in_cnt_host", c_void_p),
                ("slot_shared", c_void_p), ("slot_stride", c_int64), ("dup_bits", c_void_p), ("dup_words", c_int64),
                ("cidx", c_void_p), ("rows", c_void_p), ("row_cap", c_int64), ("counts", c_void_p)]


class ShardBufs(Structure):
    """hiprec_shard_bufs (include/hiprec.h)."""

    _fields_ = [("w_flat", c_void_p), ("n_users_local", c_int64), ("n_items_local", c_int64), ("dim", c_int32),
                ("_pad", c_int32), ("payload", c_void_p), ("g_recv", c_void_p), ("fetched", c_void_p),
                ("g_send", c_void_p), ("arrived", c_void_p), ("acc", c_void_p), ("scratch", c_void_p),
                ("g_flat", c_void_p), ("m_flat", c_void_p), ("v_flat", c_void_p),
                ("stamp_u", c_void_p), ("stamp_i", c_void_p), ("lazy_scalars", c_void_p), ("lazy_scalars_cap", c_int64),
                ("cbuf", c_void_p), ("cbias", c_void_p)]


class LazyState(Structure):
    """hiprec_lazy_state (include/hiprec.h)."""

    _fields_ = [("w", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("n_users", c_int64),
                ("n_items", c_int64), ("dim", c_int32), ("kind", c_int32), ("stamp_u", c_void_p), ("stamp_i", c_void_p),
                ("scalars", c_void_p), ("scalars_cap", c_int32), ("_pad", c_int32), ("lr", c_double),
                ("beta1", c_double), ("beta2", c_double), ("eps", c_double)]


class LazyRows(Structure):
    """hiprec_lazy_rows (include/hiprec.h)."""

    _fields_ = [("users", c_void_p), ("n_users", c_int64), ("items_a", c_void_p), ("n_items_a", c_int64),
                ("items_b", c_void_p), ("n_items_b", c_int64), ("items_c", c_void_p), ("n_items_c", c_int64)]


SHARD_EXCHANGE_SELF = 1   # include/hiprec.h HIPREC_SHARD_EXCHANGE_SELF


class NcclFns(Structure):
    """hiprec_nccl_fns (include/hiprec.h)."""

    _fields_ = [("send", c_void_p), ("recv", c_void_p), ("group_start", c_void_p), ("group_end", c_void_p)]


NGCF_MAX_LAYERS = 6


class NgcfPlan(Structure):
    """hiprec_ngcf_plan (include/hiprec.h)."""

    _fields_ = ([("a", Csr), ("at", Csr), ("n_users", c_int64), ("n_items", c_int64), ("n_layers", c_int32),
                 ("dim", c_int32 * (NGCF_MAX_LAYERS + 1)), ("decay", c_float), ("inv_reg_batch", c_float),
                 ("e0", c_void_p), ("g_e0", c_void_p)]
                + [(n, c_void_p * NGCF_MAX_LAYERS) for n in ("gc_w", "gc_b", "bi_w", "bi_b", "g_gc_w", "g_gc_b", "g_bi_w",
                                                "g_bi_b", "side", "bi_in", "sum_pre", "bi_pre", "ego", "nrm")]
                + [("all", c_void_p), ("keep", c_void_p * NGCF_MAX_LAYERS), ("keep_scale", c_float * NGCF_MAX_LAYERS),
                   ("keep_prob", c_float * NGCF_MAX_LAYERS), ("keep_seed", ctypes.c_uint64),
                   ("keep_step", ctypes.c_uint64), ("keep_gen", c_int32), ("_pad", c_int32),
                   ("d_all", c_void_p), ("d_sum", c_void_p), ("d_bi", c_void_p), ("d_side", c_void_p),
                   ("d_bi_in", c_void_p), ("d_ego", c_void_p * 2), ("spmm_tmp", c_void_p * NGCF_MAX_LAYERS),
                   ("zero_ws", c_void_p), ("zero_ws_floats", c_int64), ("sa", SlicedCsr), ("sat", SlicedCsr),
                   ("slice_w", c_int32), ("_pad2", c_int32), ("sliced_src", c_void_p),
                   ("sliced_src_floats", c_int64), ("d_sum_l", c_void_p * NGCF_MAX_LAYERS),
                   ("d_bi_l", c_void_p * NGCF_MAX_LAYERS)])


class FusedStep(Structure):
    """hiprec_fused_step (include/hiprec.h)."""

    _fields_ = [("kind", c_int32), ("dim", c_int32), ("n_users", c_int64), ("n_items", c_int64)] + \
               [(n, c_void_p) for n in ("w_read", "g_prev", "m_read", "v_read", "w_write", "m_write", "v_write",
                                        "g_cur", "g_zero", "scratch_prev", "scratch_cur")] + \
               [("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("reg_coef", c_float), ("_pad", c_int32)]


class DpStep(Structure):
    """hiprec_dp_step (include/hiprec.h)."""

    _fields_ = [("w", MfTables), ("g", MfTables), ("stats", c_void_p), ("scratch", c_void_p),
                ("scratch_bytes", c_size_t), ("loss_reg_out", c_void_p), ("w_flat", c_void_p),
                ("g_flat", c_void_p), ("m_flat", c_void_p), ("v_flat", c_void_p), ("n_flat", c_int64),
                ("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("reg_coef", c_float), ("loss_kind", c_int32), ("opt_kind", c_int32), ("_pad", c_int32)]


# name -> (restype, argtypes); every symbol of include/hiprec.h must be listed here
_P = c_void_p
_T = POINTER(MfTables)
SIGNATURES = {
    "hiprec_version": (c_int, []),
    "hiprec_source_hash": (ctypes.c_char_p, []),
    "hiprec_last_error": (c_char_p, []),
    "hiprec_stats_bytes": (c_size_t, []),
    "hiprec_scratch_bytes": (c_size_t, [c_int64]),
    "hiprec_stats_reset": (c_int, [_P, c_double, c_double, _P]),
    "hiprec_stats_advance_step": (c_int, [_P, _P]),
    "hiprec_stats_set_step": (c_int, [_P, c_int64, c_double, c_double, _P]),
    "hiprec_stats_begin_epoch": (c_int, [_P, _P]),
    "hiprec_gather_rows": (c_int, [_P, c_int64, c_int32, _P, c_int64, _P, _P, _P]),
    "hiprec_route_bucket": (c_int, [_P, c_int64, c_int32, c_int64, _P, _P, _P, _P]),
    "hiprec_shard_route_triples": (c_int, [_P, _P, _P, c_int64, c_int32, c_int64, _P, _P, _P, _P]),
    "hiprec_shard_route_items": (c_int, [_P, c_int64, c_int32, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "hiprec_shard_gather_payload": (c_int, [_P, _P, c_int64, c_int32, _P, c_int64, c_int32, _P, _P, _P, _P]),
    "hiprec_shard_split_rows": (c_int, [_P, c_int64, c_int32, _P, _P, _P]),
    "hiprec_shard_join_rows": (c_int, [_P, _P, c_int64, c_int32, _P, _P]),
    "hiprec_scatter_add_rows": (c_int, [_P, c_int64, c_int32, _P, _P, c_int64, c_int64, _P, _P]),
    "hiprec_mf_predict": (c_int, [_T, _P, _P, c_int64, _P, _P, _P]),
    "hiprec_mf_forward": (c_int, [_T, _P, _P, c_int64, _P, _P, _P, _P]),
    "hiprec_mf_bpr_grad": (
        c_int,
        [_T, _T, _P, _P, _P, _P, c_int64, c_float, c_float, _P, _P, c_size_t, _P],
    ),
    "hiprec_mf_bce_grad": (
        c_int,
        [_T, _T, _P, _P, _P, _P, c_int64, c_float, c_float, _P, _P, c_size_t, _P],
    ),
    "hiprec_finalize_stats": (c_int, [_P, _P, _P, _P, _P]),
    "hiprec_opt_dense_step": (
        c_int,
        [c_int, _P, _P, _P, _P, c_int64, c_double, c_double, c_double, c_double, _P, _P, c_int64,
         _P],
    ),
    "hiprec_mf_sgd_rows": (
        c_int,
        [_T, _T, _P, _P, _P, _P, c_int64, c_double, _P, _P, c_int32, _P, _P, _P],
    ),
    "hiprec_ncf_plan_bytes": (c_size_t, []),
    "hiprec_gemm_f32": (
        c_int,
        [c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P],
    ),
    "hiprec_ncf_forward": (c_int, [POINTER(NcfPlan), _P, _P, c_int64, _P, _P]),
    "hiprec_ncf_grad": (
        c_int,
        [POINTER(NcfPlan), _P, _P, _P, c_int64, c_float, _P, _P, c_size_t, _P],
    ),
    "hiprec_ncf_step": (
        c_int,
        [POINTER(NcfPlan), _P, _P, _P, c_int64, c_float, c_int, _P, _P, _P, _P, c_int64, c_int64, c_int64, c_double,
         c_double, c_double, c_double, _P, _P, c_size_t, _P],
    ),
    "hiprec_lightgcn_plan_bytes": (c_size_t, []),
    "hiprec_spmm_csr": (c_int, [POINTER(Csr), _P, c_float, _P, _P, _P, c_int32, _P]),
    "hiprec_sliced_width": (c_int32, [c_int64, c_int32]),
    "hiprec_sliced_row_cap": (c_int32, [c_int64, c_int32]),
    "hiprec_to_sliced": (c_int, [_P, c_int64, c_int32, c_int32, _P, _P, _P]),
    "hiprec_from_sliced": (c_int, [_P, c_int64, c_int32, c_int32, _P, c_int32, _P]),
    "hiprec_sliced_drop_values": (c_int, [POINTER(SlicedCsr), _P, _P, _P]),
    "hiprec_spmm_sliced": (c_int, [POINTER(SlicedCsr), _P, c_float, _P, _P, _P, c_int32, c_int32, c_int32, _P]),
    "hiprec_edge_dropout_mask": (c_int, [_P, c_int64, c_float, ctypes.c_uint64, ctypes.c_uint64, _P]),
    "hiprec_lightgcn_step_values": (c_int, [POINTER(LightGcnPlan), _P, c_float, c_int32, ctypes.c_uint64,
                                            ctypes.c_uint64, _P]),
    "hiprec_lightgcn_opt_stage": (c_int, [POINTER(LightGcnPlan), c_int32, _P, _P, _P, c_double, c_double, c_double,
                                          c_double, _P, _P, c_float, ctypes.c_uint64, ctypes.c_uint64, _P]),
    "hiprec_lightgcn_propagate": (c_int, [POINTER(LightGcnPlan), _P, c_float, _P]),
    "hiprec_lightgcn_predict": (c_int, [POINTER(LightGcnPlan), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_lightgcn_grad": (
        c_int,
        [POINTER(LightGcnPlan), _P, c_float, _P, _P, _P, c_int64, c_float, _P, _P, c_size_t, _P],
    ),
    "hiprec_random_permutation": (c_int, [_P, c_int64, ctypes.c_uint64, _P]),
    "hiprec_fused_step_bytes": (c_size_t, []),
    "hiprec_mf_bpr_fused_step": (c_int, [POINTER(FusedStep), _P, _P, _P, c_int64, c_int64, c_float, _P, _P]),
    "hiprec_dp_step_bytes": (c_size_t, []),
    "hiprec_mf_dp_step_begin": (c_int, [POINTER(DpStep), _P, _P, _P, c_int64, c_float, _P]),
    "hiprec_mf_dp_step_end": (c_int, [POINTER(DpStep), _P]),
    "hiprec_sample_negatives": (
        c_int,
        [_P, _P, c_int64, c_int64, _P, c_int64, c_int32, ctypes.c_uint64, _P, _P, _P],
    ),
    "hiprec_pgmf_workspace_bytes": (c_size_t, [c_int32]),
    "hiprec_pgmf_bpr_grad": (
        c_int,
        [POINTER(PgmfTables), POINTER(PgmfTables), _P, _P, _P, c_int64, c_float, c_float, _P, _P, c_size_t,
         _P, c_size_t, _P],
    ),
    "hiprec_pgmf_epoch": (
        c_int,
        [POINTER(PgmfTables), POINTER(PgmfTables), _P, _P, _P, c_int64, c_int64, c_float, c_float, c_int,
         c_double, c_double, c_double, c_double, _P, _P, _P, _P, c_int64, _P, _P, c_size_t, _P, c_size_t,
         _P, c_size_t, _P],
    ),
    "hiprec_cmn_tables_bytes": (c_size_t, []),
    "hiprec_cmn_workspace_bytes": (c_size_t, [c_int32, c_int64]),
    "hiprec_cmn_grad_padded": (
        c_int,
        [POINTER(CmnTables), POINTER(CmnTables), _P, _P, _P, _P, _P, c_int64, _P, _P, c_int64, c_int64, c_float,
         c_float, _P, _P, _P, _P, c_size_t, _P, c_size_t, _P],
    ),
    "hiprec_cmn_grad_csr": (
        c_int,
        [POINTER(CmnTables), POINTER(CmnTables), _P, _P, _P, _P, _P, c_int64, c_float, c_float, _P, _P, _P, _P,
         c_size_t, _P, c_size_t, _P],
    ),
    "hiprec_cmn_epoch": (
        c_int,
        [POINTER(CmnTables), POINTER(CmnTables), _P, _P, _P, _P, _P, c_int64, c_int64, c_float, c_float, c_int,
         c_double, c_double, c_double, c_double, _P, _P, _P, _P, c_int64, _P, _P, c_size_t, _P, c_size_t,
         _P, c_size_t, _P],
    ),
    "hiprec_t2v_epoch": (
        c_int,
        [POINTER(T2vTables), POINTER(T2vTables), _P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int32, c_float,
         c_int, c_double, c_double, c_double, c_double, _P, _P, _P, _P, c_int64, _P, _P, c_size_t, _P],
    ),
    "hiprec_clip_workspace_bytes": (c_size_t, []),
    "hiprec_clip_grad_norm": (c_int, [_P, c_int64, c_float, _P, c_size_t, _P]),
    "hiprec_clip_opt_dense_step": (
        c_int,
        [c_int, _P, _P, _P, _P, c_int64, c_double, c_double, c_double, c_double, _P, _P, c_int64, c_float, _P, c_size_t,
         _P],
    ),
    "hiprec_t2v_grad": (
        c_int,
        [POINTER(T2vTables), POINTER(T2vTables), _P, _P, _P, _P, _P, _P, c_int64, c_int32, c_float, _P, _P,
         c_size_t, _P],
    ),
    "hiprec_t2v_predict": (c_int, [POINTER(T2vTables), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_sumsq_workspace_bytes": (c_size_t, []),
    "hiprec_sumsq": (c_int, [_P, c_int64, _P, c_size_t, _P]),
    "hiprec_opt_dense_step_decay": (
        c_int,
        [c_int, _P, _P, _P, _P, c_int64, c_double, c_double, c_double, c_double, _P, _P, c_float, _P, c_size_t, _P],
    ),
    "hiprec_decay_grad": (c_int, [_P, _P, c_int64, c_float, _P]),
    "hiprec_ultragcn_grad": (
        c_int,
        [POINTER(UltraGcnTables), POINTER(UltraGcnTables), POINTER(UltraGcnParams), _P, _P, _P, c_int64, c_int32, _P,
         _P, _P, c_size_t, _P],
    ),
    "hiprec_ultragcn_predict": (c_int, [POINTER(UltraGcnTables), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_ultragcn_epoch": (
        c_int,
        [POINTER(UltraGcnTables), POINTER(UltraGcnTables), POINTER(UltraGcnParams), _P, _P, _P, c_int64, c_int64,
         c_int32, c_int, c_double, c_double, c_double, c_double, _P, _P, _P, _P, c_int64, _P, c_size_t, _P, _P,
         c_size_t, _P],
    ),
    "hiprec_mixgcf_plan_bytes": (c_size_t, []),
    "hiprec_mixgcf_propagate": (c_int, [POINTER(MixGcfPlan), c_int32, _P]),
    "hiprec_mixgcf_predict": (c_int, [POINTER(MixGcfPlan), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_mixgcf_grad": (
        c_int,
        [POINTER(MixGcfPlan), _P, _P, _P, c_int64, c_int64, _P, _P, c_float, _P, _P, c_size_t, _P],
    ),
    "hiprec_sgl_plan_bytes": (c_size_t, []),
    "hiprec_sgl_tile_b": (c_int32, []),
    "hiprec_sgl_tile_n": (c_int32, []),
    "hiprec_sgl_ws_floats": (c_int64, [c_int64, c_int32]),
    "hiprec_sgl_batch_ws_floats": (c_int64, [c_int64, c_int32]),
    "hiprec_sgl_sub_values": (c_int, [POINTER(Csr), _P, _P, _P, _P, c_int64, _P, _P, _P]),
    "hiprec_sgl_propagate": (c_int, [POINTER(SglPlan), _P]),
    "hiprec_sgl_predict": (c_int, [POINTER(SglPlan), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_sgl_grad": (c_int, [POINTER(SglPlan), _P, _P, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "hiprec_lcfn_plan_bytes": (c_size_t, []),
    "hiprec_lcfn_tile_rows": (c_int32, []),
    "hiprec_lcfn_max_slots": (c_int32, []),
    "hiprec_lcfn_loss_triples_per_block": (c_int32, []),
    "hiprec_lcfn_ws_floats": (c_int64, [c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "hiprec_lcfn_batch_ws_floats": (c_int64, [c_int64]),
    "hiprec_lcfn_propagate": (c_int, [POINTER(LcfnPlan), _P]),
    "hiprec_lcfn_predict": (c_int, [POINTER(LcfnPlan), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_lcfn_grad": (c_int, [POINTER(LcfnPlan), _P, _P, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "hiprec_simgcl_plan_bytes": (c_size_t, []),
    "hiprec_simgcl_tile_b": (c_int32, []),
    "hiprec_simgcl_tile_n": (c_int32, []),
    "hiprec_simgcl_max_dim": (c_int32, []),
    "hiprec_simgcl_max_layers": (c_int32, []),
    "hiprec_simgcl_ws_floats": (c_int64, [c_int64, c_int32]),
    "hiprec_simgcl_stamp_ints": (c_int64, [c_int64]),
    "hiprec_simgcl_batch_ws_floats": (c_int64, [c_int64, c_int32]),
    "hiprec_simgcl_noise": (c_int, [c_uint64, c_uint64, c_int32, c_int64, c_int32, _P, _P]),
    "hiprec_simgcl_predict": (c_int, [POINTER(SimgclPlan), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_simgcl_grad": (c_int, [POINTER(SimgclPlan), _P, _P, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "hiprec_buir_plan_bytes": (c_size_t, []),
    "hiprec_buir_tile_b": (c_int32, []),
    "hiprec_buir_max_dim": (c_int32, []),
    "hiprec_buir_max_layers": (c_int32, []),
    "hiprec_buir_ws_floats": (c_int64, [c_int64, c_int32]),
    "hiprec_buir_batch_ws_floats": (c_int64, [c_int64, c_int32]),
    "hiprec_buir_pool": (c_int, [POINTER(BuirPlan), _P, _P, _P, _P]),
    "hiprec_buir_grad": (c_int, [POINTER(BuirPlan), _P, _P, _P, c_int64, _P, _P, c_size_t, _P]),
    "hiprec_buir_ema": (c_int, [POINTER(BuirPlan), _P]),
    "hiprec_buir_predict": (c_int, [POINTER(BuirPlan), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_sasrec_shape_bytes": (c_size_t, []),
    "hiprec_sasrec_param_floats": (c_int64, [POINTER(SasrecShape)]),
    "hiprec_sasrec_workspace_bytes": (c_size_t, [POINTER(SasrecShape), c_int64, c_int32]),
    "hiprec_sasrec_grad": (
        c_int,
        [POINTER(SasrecShape), _P, _P, _P, _P, _P, c_int64, c_int32, c_float, _P, c_float, _P, _P, _P, c_size_t, _P,
         c_size_t, _P],
    ),
    "hiprec_tisasrec_shape_bytes": (c_size_t, []),
    "hiprec_tisasrec_param_floats": (c_int64, [POINTER(TisasrecShape)]),
    "hiprec_tisasrec_workspace_bytes": (c_size_t, [POINTER(TisasrecShape), c_int64, c_int32]),
    "hiprec_tisasrec_grad": (
        c_int,
        [POINTER(TisasrecShape), _P, _P, _P, _P, _P, _P, c_int64, c_int32, c_float, _P, c_float, _P, _P, _P, c_size_t,
         _P, c_size_t, _P],
    ),
    "hiprec_bert4rec_shape_bytes": (c_size_t, []),
    "hiprec_bert4rec_param_floats": (c_int64, [POINTER(Bert4recShape)]),
    "hiprec_bert4rec_workspace_bytes": (c_size_t, [POINTER(Bert4recShape), c_int64, c_int32]),
    "hiprec_bert4rec_grad": (
        c_int,
        [POINTER(Bert4recShape), _P, _P, _P, c_int64, _P, _P, c_int64, c_int32, _P, c_float, _P, _P, _P, c_size_t, _P,
         c_size_t, _P],
    ),
    "hiprec_bert4rec_head": (c_int, [POINTER(Bert4recShape), _P, _P, c_int64, _P, _P, c_size_t, _P]),
    "hiprec_narm_shape_bytes": (c_size_t, []),
    "hiprec_narm_param_floats": (c_int64, [POINTER(NarmShape)]),
    "hiprec_narm_workspace_bytes": (c_size_t, [POINTER(NarmShape), c_int64, c_int32]),
    "hiprec_narm_grad": (
        c_int,
        [POINTER(NarmShape), _P, _P, _P, _P, _P, c_int64, c_int32, _P, c_float, c_float, _P, _P, _P, c_size_t, _P,
         c_size_t, _P],
    ),
    "hiprec_caser_shape_bytes": (c_size_t, []),
    "hiprec_caser_param_floats": (c_int64, [POINTER(CaserShape)]),
    "hiprec_caser_workspace_bytes": (c_size_t, [POINTER(CaserShape), c_int64]),
    "hiprec_caser_grad": (
        c_int,
        [POINTER(CaserShape), _P, _P, _P, _P, _P, _P, c_int64, _P, c_float, c_float, _P, _P, _P, c_size_t, _P, c_size_t,
         _P],
    ),
    "hiprec_caser_score": (c_int, [POINTER(CaserShape), _P, _P, _P, c_int64, c_int32, _P, _P, _P]),
    "hiprec_gru4rec_shape_bytes": (c_size_t, []),
    "hiprec_gru4rec_param_floats": (c_int64, [POINTER(Gru4recShape)]),
    "hiprec_gru4rec_workspace_bytes": (c_size_t, [POINTER(Gru4recShape), c_int64, c_int32]),
    "hiprec_gru4rec_grad": (
        c_int,
        [POINTER(Gru4recShape), _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, _P, c_float, c_float, c_float, c_float, _P,
         c_float, c_float, _P, _P, _P, c_size_t, _P, c_size_t, _P],
    ),
    "hiprec_srgnn_shape_bytes": (c_size_t, []),
    "hiprec_srgnn_param_floats": (c_int64, [POINTER(SrgnnShape)]),
    "hiprec_srgnn_workspace_bytes": (c_size_t, [POINTER(SrgnnShape), c_int64, c_int32, c_int64]),
    "hiprec_srgnn_graph_ints": (c_int64, [c_int64, c_int32, c_int64]),
    "hiprec_srgnn_graph": (c_int, [POINTER(SrgnnShape), _P, _P, c_int64, c_int32, c_int64, _P, c_size_t, _P, _P]),
    "hiprec_srgnn_grad": (
        c_int,
        [POINTER(SrgnnShape), _P, _P, _P, _P, _P, c_int64, c_int32, c_int64, c_float, _P, _P, _P, c_size_t, _P, c_size_t,
         _P],
    ),
    "hiprec_vbcar_shape_bytes": (c_size_t, []),
    "hiprec_vbcar_param_floats": (c_int64, [POINTER(VbcarShape)]),
    "hiprec_vbcar_workspace_bytes": (c_size_t, [POINTER(VbcarShape), c_int64, c_int32]),
    "hiprec_vbcar_encode_workspace_bytes": (c_size_t, [POINTER(VbcarShape), c_int64, c_int32]),
    "hiprec_vbcar_grad": (
        c_int,
        [POINTER(VbcarShape), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, _P, c_float, c_float, _P, _P,
         c_size_t, _P, c_size_t, _P],
    ),
    "hiprec_vbcar_encode": (c_int, [POINTER(VbcarShape), _P, _P, _P, c_int64, c_int32, _P, _P, _P, c_size_t, _P]),
    "hiprec_vbcar_predict": (c_int, [POINTER(VbcarShape), _P, _P, _P, _P, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "hiprec_tvbr_shape_bytes": (c_size_t, []),
    "hiprec_tvbr_param_floats": (c_int64, [POINTER(TvbrShape)]),
    "hiprec_tvbr_workspace_bytes": (c_size_t, [POINTER(TvbrShape), c_int64, c_int32]),
    "hiprec_tvbr_encode_workspace_bytes": (c_size_t, [POINTER(TvbrShape), c_int64, c_int32]),
    "hiprec_tvbr_grad": (
        c_int,
        [POINTER(TvbrShape), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, _P, c_float, c_float, _P,
         _P, c_size_t, _P, c_size_t, _P],
    ),
    "hiprec_tvbr_encode": (c_int, [POINTER(TvbrShape), _P, _P, _P, c_int64, c_int32, _P, _P, _P, c_size_t, _P]),
    "hiprec_tvbr_predict": (c_int, [POINTER(TvbrShape), _P, _P, _P, _P, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "hiprec_vaecf_shape_bytes": (c_size_t, []),
    "hiprec_vaecf_param_floats": (c_int64, [POINTER(VaecfShape)]),
    "hiprec_vaecf_workspace_bytes": (c_size_t, [POINTER(VaecfShape), c_int64, c_int64]),
    "hiprec_vaecf_encode_workspace_bytes": (c_size_t, [POINTER(VaecfShape), c_int64]),
    "hiprec_vaecf_decode_workspace_bytes": (c_size_t, [POINTER(VaecfShape), c_int64]),
    "hiprec_vaecf_grad": (
        c_int,
        [POINTER(VaecfShape), _P, _P, _P, _P, _P, c_int64, c_int64, _P, c_float, _P, _P, c_size_t, _P, c_size_t, _P],
    ),
    "hiprec_vaecf_encode": (c_int, [POINTER(VaecfShape), _P, _P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "hiprec_vaecf_decode_at": (
        c_int, [POINTER(VaecfShape), _P, _P, c_int64, _P, _P, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "hiprec_time_relation": (c_int, [_P, c_int64, c_int32, c_int32, _P, _P]),
    "hiprec_alias_sample": (c_int, [_P, _P, _P, c_int64, ctypes.c_uint64, _P, c_int64, _P]),
    "hiprec_ngcf_plan_bytes": (c_size_t, []),
    "hiprec_ngcf_forward": (c_int, [POINTER(NgcfPlan), c_int, _P]),
    "hiprec_ngcf_predict": (c_int, [POINTER(NgcfPlan), _P, _P, c_int64, _P, _P, _P]),
    "hiprec_ngcf_grad": (c_int, [POINTER(NgcfPlan), _P, _P, _P, c_int64, c_float, _P, _P, c_size_t, _P]),
    "hiprec_csr_n_slices": (c_int64, [c_int64]),
    "hiprec_csr_slice_rows": (c_int, [POINTER(Csr), _P, c_int64, _P]),
    "hiprec_rank_metrics_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "hiprec_rank_metrics": (
        c_int,
        [_P, c_int64, _P, _P, POINTER(c_int32), c_int32, _P, c_size_t, _P, _P],
    ),
    "hiprec_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "hiprec_topk_recommend": (
        c_int,
        [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int32, c_float, _P, _P, c_int64, _P, _P, c_int32, c_int32, _P,
         c_size_t, _P, _P, _P, _P],
    ),
    "hiprec_topk_metrics": (
        c_int,
        [_P, c_int64, c_int32, _P, _P, POINTER(c_int32), c_int32, _P, c_size_t, _P, _P],
    ),
    "hiprec_knn_workspace_bytes": (c_size_t, [c_int32, c_int64, c_int64, c_int64, c_int32]),
    "hiprec_knn_item_similarity": (
        c_int, [_P, _P, _P, _P, _P, _P, c_int64, c_int64, _P, c_int64, c_int32, _P, c_size_t, _P]),
    "hiprec_knn_item_scores": (
        c_int,
        [_P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, c_int32, _P, _P, _P, _P, c_int32, _P, c_size_t,
         _P, _P],
    ),
    "hiprec_knn_user_scores": (
        c_int,
        [_P, _P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int32, _P, c_int64, _P, _P, _P, _P, _P, c_int32, _P, _P, _P, _P,
         c_int32, _P, c_size_t, _P, _P],
    ),
    "hiprec_als_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32]),
    "hiprec_als_gram": (c_int, [_P, c_int64, c_int32, c_float, _P, _P, _P, c_size_t, _P]),
    "hiprec_als_solve_rows": (
        c_int, [_P, _P, _P, _P, c_int64, _P, c_int64, c_int32, _P, c_float, _P, c_int32, _P, _P, _P]),
    "hiprec_als_loss": (
        c_int, [_P, _P, _P, c_int64, _P, _P, c_int64, c_int32, _P, c_float, c_float, _P, c_size_t, _P, _P, _P]),
    "hiprec_ease_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "hiprec_ease_gram": (
        c_int, [_P, _P, _P, _P, c_int64, c_int64, c_float, _P, c_int32, _P, c_size_t, _P, _P]),
    "hiprec_ease_invert": (c_int, [_P, c_int64, _P, c_size_t, _P, _P]),
    "hiprec_ease_finish": (c_int, [_P, c_int64, _P, _P, _P]),
    "hiprec_slim_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "hiprec_slim_fit": (
        c_int, [_P, c_int64, c_float, c_int32, c_float, c_int32, _P, _P, c_int32, _P, c_size_t, _P, _P]),
    "hiprec_stage_epoch": (c_int, [_P, _P, _P, c_int32, _P, c_int64, c_int64, _P, _P, _P, _P]),
    "hiprec_stage_epoch_shuffled": (c_int, [_P, _P, _P, c_int32, ctypes.c_uint64, c_int64, c_int64, _P, _P, _P, _P]),
    "hiprec_mf_bce_epoch": (
        c_int,
        [_T, _T, _P, _P, _P, _P, c_int64, c_int64, c_float, c_int]
        + [c_double, c_double, c_double, c_double]
        + [_P, _P, _P, _P, c_int64, _P, _P, c_int32, _P, _P, c_size_t, _P],
    ),
    "hiprec_mf_bpr_epoch_fused": (
        c_int,
        [c_int, _P, _P, _P, _P, _P, c_int64, c_int64, c_int32, _P, _P, _P, c_int64, c_int64, c_float,
         c_double, c_double, c_double, c_double, _P, POINTER(c_int32), _P],
    ),
    "hiprec_mf_bpr_epoch_fused_range": (
        c_int,
        [c_int, _P, _P, _P, _P, _P, c_int64, c_int64, c_int32, _P, _P, _P, c_int64, c_int64, c_int64, c_int64,
         c_float, c_double, c_double, c_double, c_double, _P, POINTER(c_int32), _P],
    ),
    "hiprec_mf_bpr_dp_epoch_fused_range": (
        c_int,
        [c_int, _P, _P, c_int64, _P, _P, c_int64, c_int64, c_int64, c_int32, _P, _P, _P, c_int64, c_int64, c_int64,
         c_int64, c_int32, c_float, c_double, c_double, c_double, c_double, _P, _P, _P, POINTER(c_int32), _P],
    ),
    "hiprec_mf_bpr_epoch_owned": (
        c_int,
        [_P, c_int64, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P, c_int64, _P, _P, c_int64, _P, _P, c_int64,
         c_int64, c_int64, c_int64, c_float, c_double, _P, _P],
    ),
    "hiprec_ownership_table_bits": (c_int32, [c_int64]),
    "hiprec_ownership_ws_ints": (c_int64, [c_int64, c_int64, c_int32]),
    "hiprec_batch_row_ownership": (
        c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int64, c_int32, _P, _P, _P, _P]),
    "hiprec_stage_grouped_ws_ints": (c_int64, [c_int64, c_int64, c_int64]),
    "hiprec_stage_epoch_grouped": (
        c_int, [_P, _P, _P, _P, c_int32, ctypes.c_uint64, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "hiprec_mf_pull_chunk": (c_int32, [c_int32]),
    "hiprec_contrib_row_cap": (c_int64, [c_int64, c_int32]),
    "hiprec_batch_row_contrib": (
        c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, _P, _P, _P, c_int64, _P, _P]),
    "hiprec_mf_bpr_epoch_pull": (
        c_int,
        [_P, c_int64, c_int64, c_int32, _P, _P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, c_int64, c_int64,
         c_int64, c_int64, c_float, c_double, _P, _P],
    ),
    "hiprec_mf_bpr_owned_remote_step": (
        c_int,
        [_P, c_int64, c_int64, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_float,
         c_float, c_double, _P, _P, _P],
    ),
    "hiprec_mf_bpr_pull_remote_step": (
        c_int,
        [_P, c_int64, c_int64, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, c_int64, _P, _P, _P, _P, c_int32,
         c_int64, c_float, c_float, c_double, _P, _P, _P],
    ),
    "hiprec_batch_row_ownership_tables": (
        c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "hiprec_plan_route_tiles": (c_int64, [c_int64, c_int64]),
    "hiprec_plan_route_triples": (
        c_int, [_P, _P, _P, _P, c_int64, c_int64, c_int32, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "hiprec_plan_place_triples": (c_int, [_P, c_int64, _P, c_int32, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "hiprec_plan_slot_ws_ints": (c_int64, [c_int64, c_int32, c_int32]),
    "hiprec_plan_item_slots": (
        c_int, [_P, c_int64, c_int64, c_int32, c_int64, c_int32] + [_P] * 16 + [_P, _P, c_int64, _P, _P]),
    "hiprec_plan_place_requests": (c_int, [_P, c_int64, _P, c_int32, c_int64, _P, _P, _P, _P, c_int64, _P, _P]),
    "hiprec_shard_payload_zero": (
        c_int, [_P, _P, c_int64, c_int32, _P, c_int64, c_int64, c_int64, _P, _P, _P, c_int64, _P, _P, _P]),
    "hiprec_mf_bpr_grad_remote_step": (
        c_int,
        [_P, _P, c_int64, c_int64, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, c_int64, c_float, c_float,
         _P, _P, _P],
    ),
    "hiprec_shard_apply_finish": (
        c_int, [_P, _P, c_int64, c_int32, _P, _P, c_int64, c_int64, c_int64, _P, c_double, _P, c_int32, _P, c_double,
                c_int32, _P, _P, _P]),
    "hiprec_shard_planned_steps": (
        c_int, [POINTER(ShardPlan), POINTER(ShardBufs), c_int64, c_int64, c_int32, c_float, c_double, c_double,
                c_double, c_double, POINTER(NcclFns), _P, _P, _P]),
    "hiprec_shard_planned_steps_ex": (
        c_int, [POINTER(ShardPlan), POINTER(ShardBufs), c_int64, c_int64, c_int32, c_float, c_double, c_double,
                c_double, c_double, POINTER(NcclFns), _P, ctypes.c_uint32, _P, _P]),
    "hiprec_gather_epoch": (c_int, [_P, _P, _P, _P, c_int32, ctypes.c_uint64, _P, c_int64, _P, _P, _P, _P]),
    "hiprec_stage_sort_keys": (c_int, [_P, _P, c_int32, ctypes.c_uint64, c_int64, c_int64, c_int64, c_int32, _P, _P]),
    "hiprec_group_epoch_by_item": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P, _P,
                                           _P, _P]),
    "hiprec_lazy_state_bytes": (c_size_t, []),
    "hiprec_lazy_catchup": (c_int, [POINTER(LazyState), POINTER(LazyRows), _P, _P]),
    "hiprec_lazy_update": (c_int, [POINTER(LazyState), POINTER(LazyRows), _P, _P, _P]),
    "hiprec_lazy_flush": (c_int, [POINTER(LazyState), _P, _P]),
    "hiprec_lazy_mark_current": (c_int, [POINTER(LazyState), _P, _P]),
    "hiprec_mf_epoch_lazy": (c_int, [POINTER(LazyState), _T, _T, _P, _P, _P, c_int32, c_int64, c_int64, c_int32, c_float,
                                     _P, _P, c_size_t, _P]),
    "hiprec_mf_bpr_grad_owned": (c_int, [_P, _P, c_int64, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P, c_int64, c_float,
                                         c_float, _P, _P, _P]),
    "hiprec_mf_epoch_lazy_pull": (c_int, [POINTER(LazyState), _P, _P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, c_int64,
                                          c_int64, c_int32, c_float, _P, _P, _P]),
    "hiprec_mf_epoch_lazy_owned": (c_int, [POINTER(LazyState), _P, _P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int64,
                                           c_int32, c_float, _P, _P, _P]),
    "hiprec_shard_plan_bytes": (c_size_t, []),
    "hiprec_shard_bufs_bytes": (c_size_t, []),
    "hiprec_shard_publish_partials": (c_int, [_P, _P, c_int32, _P, c_int32, _P]),
    "hiprec_shard_apply_rows": (c_int, [_P, _P, c_int64, c_int32, _P, _P, c_int64, c_double, _P, _P]),
    "hiprec_shard_finish_step": (c_int, [_P, c_int32, _P, c_int32, _P, c_double, c_int32, _P, _P]),
    "hiprec_mf_bpr_epoch_sgd_fused": (
        c_int,
        [_P, _P, _P, c_int64, c_int64, c_int32, _P, _P, _P, c_int64, c_int64, c_float, c_double, _P,
         POINTER(c_int32), _P],
    ),
    "hiprec_mf_bpr_epoch": (
        c_int,
        [_T, _T, _P, _P, _P, _P, c_int64, c_int64, c_float, c_int]
        + [c_double, c_double, c_double, c_double]
        + [_P, _P, _P, _P, c_int64, _P, _P, c_int32, _P, _P, c_size_t, _P],
    ),
}

_lib = None


class HiprecError(RuntimeError):
    """A libhiprec call returned a non-zero code."""


def load():
    """Load libhiprec.so (once) and attach the prototypes.  Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libhiprec.so not found at {LIB_PATH}: the HIP extension is the only compute path of "
            "this package (there is no CPU fallback). Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)."
        )
    # torch must be imported first so that libamdhip64.so.7 resolves to the runtime torch already
    # loaded (one HIP runtime per process: streams and device pointers are shared with torch).
    import torch  # noqa: F401

    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise RuntimeError(f"libhiprec.so does not export {name}; rebuild it") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.hiprec_stats_bytes() != ctypes.sizeof(Stats):
        raise RuntimeError("hiprec_stats layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_lightgcn_plan_bytes() != ctypes.sizeof(LightGcnPlan):
        raise RuntimeError("hiprec_lightgcn_plan layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_fused_step_bytes() != ctypes.sizeof(FusedStep):
        raise RuntimeError("hiprec_fused_step layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_dp_step_bytes() != ctypes.sizeof(DpStep):
        raise RuntimeError("hiprec_dp_step layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_ngcf_plan_bytes() != ctypes.sizeof(NgcfPlan):
        raise RuntimeError("hiprec_ngcf_plan layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_lazy_state_bytes() != ctypes.sizeof(LazyState):
        raise RuntimeError("hiprec_lazy_state layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_shard_bufs_bytes() != ctypes.sizeof(ShardBufs):
        raise RuntimeError("hiprec_shard_bufs layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_cmn_tables_bytes() != ctypes.sizeof(CmnTables):
        raise RuntimeError("hiprec_cmn_tables layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_sasrec_shape_bytes() != ctypes.sizeof(SasrecShape):
        raise RuntimeError("hiprec_sasrec_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_tisasrec_shape_bytes() != ctypes.sizeof(TisasrecShape):
        raise RuntimeError("hiprec_tisasrec_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_bert4rec_shape_bytes() != ctypes.sizeof(Bert4recShape):
        raise RuntimeError("hiprec_bert4rec_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_narm_shape_bytes() != ctypes.sizeof(NarmShape):
        raise RuntimeError("hiprec_narm_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_caser_shape_bytes() != ctypes.sizeof(CaserShape):
        raise RuntimeError("hiprec_caser_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_gru4rec_shape_bytes() != ctypes.sizeof(Gru4recShape):
        raise RuntimeError("hiprec_gru4rec_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_srgnn_shape_bytes() != ctypes.sizeof(SrgnnShape):
        raise RuntimeError("hiprec_srgnn_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_vbcar_shape_bytes() != ctypes.sizeof(VbcarShape):
        raise RuntimeError("hiprec_vbcar_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_tvbr_shape_bytes() != ctypes.sizeof(TvbrShape):
        raise RuntimeError("hiprec_tvbr_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_vaecf_shape_bytes() != ctypes.sizeof(VaecfShape):
        raise RuntimeError("hiprec_vaecf_shape layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_mixgcf_plan_bytes() != ctypes.sizeof(MixGcfPlan):
        raise RuntimeError("hiprec_mixgcf_plan layout mismatch between _lib.py and libhiprec.so")
    if lib.hiprec_sgl_plan_bytes() != ctypes.sizeof(SglPlan):
        raise RuntimeError("hiprec_sgl_plan layout mismatch between _lib.py and libhiprec.so")
    if (lib.hiprec_sgl_tile_b(), lib.hiprec_sgl_tile_n()) != (SGL_TILE_B, SGL_TILE_N):
        raise RuntimeError("SGL tile sizes differ between _lib.py and libhiprec.so")
    if lib.hiprec_lcfn_plan_bytes() != ctypes.sizeof(LcfnPlan):
        raise RuntimeError("hiprec_lcfn_plan layout mismatch between _lib.py and libhiprec.so")
    if (lib.hiprec_lcfn_tile_rows(), lib.hiprec_lcfn_max_slots()) != (LCFN_TILE_ROWS, LCFN_MAX_SLOTS):
        raise RuntimeError("LCFN tile / slot constants differ between _lib.py and libhiprec.so")
    if lib.hiprec_simgcl_plan_bytes() != ctypes.sizeof(SimgclPlan):
        raise RuntimeError("hiprec_simgcl_plan layout mismatch between _lib.py and libhiprec.so")
    if (lib.hiprec_simgcl_tile_b(), lib.hiprec_simgcl_tile_n(), lib.hiprec_simgcl_max_dim(),
            lib.hiprec_simgcl_max_layers()) != (SIMGCL_TILE_B, SIMGCL_TILE_N, SIMGCL_MAX_DIM, SIMGCL_MAX_LAYERS):
        raise RuntimeError("SimGCL tile sizes / limits differ between _lib.py and libhiprec.so")
    if lib.hiprec_buir_plan_bytes() != ctypes.sizeof(BuirPlan):
        raise RuntimeError("hiprec_buir_plan layout mismatch between _lib.py and libhiprec.so")
    if (lib.hiprec_buir_tile_b(), lib.hiprec_buir_max_dim(), lib.hiprec_buir_max_layers()) != (
            BUIR_TILE_B, BUIR_MAX_DIM, BUIR_MAX_LAYERS):
        raise RuntimeError("BUIR tile size / limits differ between _lib.py and libhiprec.so")
    if lib.hiprec_ncf_plan_bytes() != ctypes.sizeof(NcfPlan):
        raise RuntimeError("hiprec_ncf_plan layout mismatch between _lib.py and libhiprec.so")
    _lib = _DeviceGuardedLib(lib)
    return _lib


class _Stream(c_void_p):
    """A hipStream_t that remembers which HIP device it belongs to (see _DeviceGuardedLib)."""

    device_index = None


class _DeviceGuardedLib:
    """libhiprec's entry points behind a HIP-device guard.

    A kernel launch goes to the CURRENT HIP device, and torch's default stream has the handle 0 on
    every device, so a call for tensors on ``cuda:1`` made while device 0 is current would run on
    GPU 0's null stream against GPU 1's pointers.  The reference never calls ``set_device`` and
    ``TrainEngine.get_device`` hands out ``cuda:N``, so every stream-taking entry point is wrapped:
    the stream argument built by :func:`stream_ptr` carries its device index, and the wrapper makes
    that device current for the duration of the call.
    """

    def __init__(self, cdll):
        self._cdll = cdll
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(cdll, name)
            setattr(self, name, self._guard(fn) if (restype is c_int and argtypes) else fn)

    @staticmethod
    def _guard(fn):
        import torch

        def call(*args):
            want = None
            for a in reversed(args):  # the stream is the last argument of almost every entry point
                if type(a) is _Stream:
                    want = a.device_index
                    break
            if want is None or want == torch.cuda.current_device():
                return fn(*args)
            with torch.cuda.device(want):
                return fn(*args)

        call.__name__ = fn.__name__
        call.argtypes, call.restype = fn.argtypes, fn.restype
        return call


def check(rc):
    """Raise HiprecError for a non-zero return code of a libhiprec call."""
    if rc != 0:
        msg = load().hiprec_last_error()  # (thread-local buffer of the C library)
        raise HiprecError(f"libhiprec call failed (code {rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a torch tensor as c_void_p (None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def stream_ptr(device):
    """Current torch stream of `device` as a hipStream_t (c_void_p)."""
    import torch

    device = torch.device(device)
    st = _Stream(torch.cuda.current_stream(device).cuda_stream)
    st.device_index = device.index if device.index is not None else torch.cuda.current_device()
    return st


LAZY_SCALARS_CAP = 1 << 16     # steps whose Adam bias corrections are tabulated for the lazy replays (csrc/lazy_opt.hip)


def lazy_betas_converge(opt, cap=LAZY_SCALARS_CAP):
    """Beyond the scalars table a lazy replay reads its LAST entry: that is only right once the bias corrections no
    longer move -- 1 - beta^t == 1.0 in double from t = cap - 1 on (default betas: t ~ 36 800).  RMSprop has no
    bias correction.  Checked when the state is set up, not after 65 536 steps of training."""
    if opt.name != "adam":
        return True
    return all(1.0 - float(b) ** (cap - 1) == 1.0 for b in (opt.beta1, opt.beta2))


def lazy_scalars_table(opt, device, cap=LAZY_SCALARS_CAP):
    """Adam's per-step scalars table [cap, 2], zero except for the last entry, which holds the CONVERGED pair
    (lr, 1): steps at or beyond the table are checked against it and replays of such steps read it -- whether or not
    step cap - 1 itself was ever taken by a lazy update (a restored clock beyond the table, or a dense sweep at that
    step, used to leave it zero: a spurious HIPREC_STATUS_LAZY_TABLE)."""
    import torch

    if not lazy_betas_converge(opt, cap):
        raise ValueError(
            f"lazy Adam tabulates the bias corrections of {cap} steps and needs them converged by then "
            f"(1 - beta^{cap - 1} == 1 in double); betas ({opt.beta1}, {opt.beta2}) do not: use dense_opt='sweep'")
    table = torch.zeros((cap, 2), dtype=torch.float32, device=device)
    if opt.name == "adam":
        # (float)(lr / (1 - 0)) and the rcp of (float)sqrt(1 - 0): exactly what a step beyond convergence derives
        table[cap - 1, 0] = float(opt.lr)
        table[cap - 1, 1] = 1.0
    return table


def lazy_state(model, g_flat, opt, device, cap=LAZY_SCALARS_CAP):
    """The lazy Adam / RMSprop state of an MF model (or a shard of one): the per-row stamps (-1 = never touched; at
    least one element, a shard may hold no rows), Adam's per-step scalars table, the ``dirty`` flag of a pending
    flush, and ``c``: the C struct that names them next to w / g / m / v."""
    import torch

    lz = {"stamp_u": torch.full((max(model.n_users, 1),), -1, dtype=torch.int32, device=device),
          "stamp_i": torch.full((max(model.n_items, 1),), -1, dtype=torch.int32, device=device),
          "scalars": lazy_scalars_table(opt, device, cap), "dirty": False}   # raises for betas it cannot tabulate
    lz["c"] = LazyState(
        model.flat.data_ptr(), g_flat.data_ptr(), opt.exp_avg.data_ptr() if opt.exp_avg is not None else None,
        opt.exp_avg_sq.data_ptr(), model.n_users, model.n_items, model.emb_dim, opt.kind, lz["stamp_u"].data_ptr(),
        lz["stamp_i"].data_ptr(), lz["scalars"].data_ptr(), cap, 0, opt.lr, opt.beta1, opt.beta2, opt.eps)
    return lz


def grow(buf, numel, dtype, device):
    """A work-space tensor of at least `numel` elements: `buf` if it is big enough (same device / dtype), else a new one.
    (Staging buffers are allocated once and kept, not re-made every epoch.)"""
    import torch

    if buf is not None and buf.numel() >= numel and buf.dtype == dtype and buf.device == torch.device(device):
        return buf
    return torch.empty(max(int(numel), 1), dtype=dtype, device=device)
