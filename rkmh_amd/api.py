"""ctypes binding of include/rkmh_amd.h (the C ABI of librkmh_amd.so).

Mirrors the reference's interface for the hot path: the mkmh free functions called from
/root/reference/src/rkmh.cpp (calc_hashes :860, minhashes :863, hash_intersection_size :869, ...) as
methods of `Context`, plus the batched replacements of main_stream's loops (:813-898, :904-948).
Fails loudly when the HIP library is missing -- there is no CPU implementation behind this module.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

FOLD_SWAP32, FOLD_H1, FOLD_W2W1 = 0, 1, 2


class RkmhError(RuntimeError):
    code = 0


class NeedFullDepthMap(RkmhError):
    """RK_ERR_NEED_FULL: a compact depth map cannot answer this input (reads with more hashes than the sketch keeps); repeat the
    pass with a full Counter."""
    code = -7


class Policy(C.Structure):
    _fields_ = [("fold", C.c_int32), ("drop_last_window", C.c_int32), ("counter_counts_zero", C.c_int32),
                ("mask_strict_less", C.c_int32), ("freq_max_inclusive", C.c_int32), ("seed", C.c_uint32),
                ("canon", C.c_int32)]
    # `canon` holds two rules (include/rkmh_amd.h): the strand rule in its low byte, the sketch rule (U6) in bit 8
    STRAND_MASK, DEDUP_DISTINCT = 0xFF, 0x100

    @property
    def strand(self):
        """The strand rule (rk_policy_strand): 0 = minhash, 1 = lexmin."""
        return self.canon & self.STRAND_MASK

    @strand.setter
    def strand(self, v):
        if not 0 <= int(v) <= self.STRAND_MASK:
            raise ValueError("strand rule outside [0, 255]")
        self.canon = (self.canon & ~self.STRAND_MASK) | int(v)

    @property
    def dedup(self):
        """The sketch rule (rk_policy_dedup): 0 = multiset (every copy of a value is kept), 1 = distinct values."""
        return 1 if self.canon & self.DEDUP_DISTINCT else 0

    @dedup.setter
    def dedup(self, v):
        self.canon = (self.canon & ~self.DEDUP_DISTINCT) | (self.DEDUP_DISTINCT if v else 0)


class CallRecord(C.Structure):
    _fields_ = [("ref", C.c_int32), ("pos", C.c_int32), ("alt_depth", C.c_int32), ("avg_d", C.c_int32), ("depth", C.c_int32),
                ("orig", C.c_uint8), ("alt", C.c_uint8), ("kind", C.c_uint8), ("pad", C.c_uint8)]


class SeqSet(C.Structure):
    _fields_ = [("nseq", C.c_int64), ("bases", C.POINTER(C.c_uint8)), ("offsets", C.POINTER(C.c_uint64)),
                ("names", C.POINTER(C.c_char)), ("name_offsets", C.POINTER(C.c_uint64)),
                ("quals", C.POINTER(C.c_char))]


def library_path():
    return os.path.join(_HERE, "lib", "librkmh_amd.so")


class IndexStats(C.Structure):
    """rk_index_stats_t: which form each key of the index took (rkmh_amd.h)"""
    _fields_ = ([(n, C.c_uint32) for n in (
        "struct_size", "keys", "buckets", "buckets_overflowed", "longest_chain", "chain_wrapped",
        "single_once", "single_multi", "pair", "list", "list_longest", "post_words",
        "kmer_form", "bases_kept", "bases_dropped_by_share_rule",
        "kv_reference", "kv_single_multi", "kv_pair", "kv_inline_list", "kv_base_inline", "kv_base_list", "kv_plain_list")]
        + [(n, C.c_uint32 * 8) for n in ("km1_bits", "km1_longest_hop", "kf4_sectors", "found")])


_u8p, _u64p, _i32p, _ip = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int)
_u32p = C.POINTER(C.c_uint32)

_SIGS = {
    "rk_default_policy": (None, [C.POINTER(Policy)]),
    "rk_policy_parse": (C.c_int, [C.c_char_p, C.POINTER(Policy)]),
    "rk_policy_describe": (C.c_int, [C.POINTER(Policy), C.c_char_p, C.c_size_t]),
    "rk_policy_same_hashes": (C.c_int, [C.POINTER(Policy), C.POINTER(Policy)]),
    "rk_policy_strand": (C.c_int, [C.POINTER(Policy)]),
    "rk_policy_dedup": (C.c_int, [C.POINTER(Policy)]),
    "rk_ctx_policy": (C.c_int, [C.c_void_p, C.POINTER(Policy)]),
    "rk_last_error": (C.c_char_p, []),
    "rk_version": (C.c_char_p, []),
    "rk_device_count": (C.c_int, []),
    "rk_ctx_create": (C.c_int, [C.c_int, C.POINTER(Policy), C.POINTER(C.c_void_p)]),
    "rk_ctx_destroy": (None, [C.c_void_p]),
    "rk_ctx_synchronize": (C.c_int, [C.c_void_p]),
    "rk_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "rk_free": (None, [C.c_void_p]),
    "rk_counter_add": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rk_counter_copy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rk_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "rk_host_free": (None, [C.c_void_p]),
    "rk_device_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "rk_device_free": (None, [C.c_void_p, C.c_void_p]),
    "rk_device_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rk_device_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rk_to_upper": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "rk_calc_hashes": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, _ip, C.c_int, C.POINTER(_u64p), _ip]),
    "rk_calc_hashes_counted": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, _ip, C.c_int, C.POINTER(_u64p), _ip, C.c_void_p]),
    "rk_calc_hash": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, _u64p]),
    "rk_minhashes": (C.c_int, [C.c_void_p, _u64p, C.c_int, C.c_int, C.POINTER(_u64p), _ip]),
    "rk_mask_by_frequency": (C.c_int, [C.c_void_p, _u64p, C.c_int, C.c_void_p, C.c_int]),
    "rk_minhashes_frequency_filter": (C.c_int, [C.c_void_p, _u64p, C.c_int, C.c_int, C.POINTER(_u64p), _ip, C.c_void_p, C.c_int, C.c_int]),
    "rk_hash_intersection_size": (C.c_int, [C.c_void_p, _u64p, C.c_int, _u64p, C.c_int, _ip]),
    "rk_hash_intersection": (C.c_int, [C.c_void_p, _u64p, C.c_int, C.c_int, _u64p, C.c_int, C.c_int, C.c_int, C.POINTER(_u64p), _ip]),
    "rk_counter_create": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_counter_wrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_counter_destroy": (None, [C.c_void_p]),
    "rk_counter_clear": (C.c_int, [C.c_void_p]),
    "rk_counter_increment": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rk_counter_get": (C.c_int, [C.c_void_p, C.c_uint64, _i32p]),
    "rk_classify_groups_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "rk_kmer_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "rk_set_kmer_form": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_index_stats": (C.c_int, [C.c_void_p, C.POINTER(IndexStats)]),
    "rk_device_props": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rk_counter_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rk_counter_load": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rk_counter_save_tagged": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32]),
    "rk_counter_load_tagged": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32]),
    "rk_depth_map_tag": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rk_counter_device_ptr": (C.c_void_p, [C.c_void_p]),
    "rk_counter_slots": (C.c_uint64, [C.c_void_p]),
    "rk_hash_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64, _ip, C.c_int, C.POINTER(_u64p), _u64p]),
    "rk_sketch_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64, _ip, C.c_int, C.c_int, _u64p, _i32p]),
    "rk_set_references": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_uint64]),
    "rk_set_reference_count_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_set_reference_sketches": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_int, _ip, C.c_int, C.c_int]),
    "rk_get_reference_sketches": (C.c_int, [C.c_void_p, _u64p, _i32p]),
    "rk_num_references": (C.c_int, [C.c_void_p]),
    "rk_set_depth_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rk_set_min_num_bound": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_set_kmer_cache": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rk_kmer_cache_state": (C.c_int, [C.c_void_p]),
    "rk_bgzf_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "rk_bgzf_close": (None, [C.c_void_p]),
    "rk_bgzf_members": (C.c_int64, [C.c_void_p]),
    "rk_bgzf_text_bytes": (C.c_uint64, [C.c_void_p]),
    "rk_bgzf_text_offset": (C.c_uint64, [C.c_void_p, C.c_int64]),
    "rk_bgzf_inflater": (C.c_char_p, []),
    "rk_bgzf_first_byte": (C.c_int, [C.c_void_p]),
    "rk_bgzf_image": (C.c_void_p, [C.c_void_p]),
    "rk_bgzf_lead_member": (C.c_int64, [C.c_void_p, C.c_int64]),
    "rk_bgzf_member": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rk_fastq_slot_set_source": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rk_host_register_readonly": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rk_host_unregister": (None, [C.c_void_p]),
    "rk_warm_up": (C.c_int, [C.c_int, C.c_int]),
    "rk_bgzf_plan": (C.c_int64, [C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.c_int64]),
    "rk_bgzf_plan_members": (C.c_int64, [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(C.c_int64), C.c_int64]),
    "rk_bgzf_fastq_records": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rk_fastq_slot_load_bgzf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rk_fasta_load_put_gzip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "rk_fasta_load_put_newline": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rk_fasta_load_put_bgzf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64]),
    "rk_gzip_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "rk_gzip_close": (None, [C.c_void_p]),
    "rk_gzip_image": (C.c_void_p, [C.c_void_p]),
    "rk_gzip_file_bytes": (C.c_uint64, [C.c_void_p]),
    "rk_gzip_first_byte": (C.c_int, [C.c_void_p]),
    "rk_gzip_text_bytes_hint": (C.c_uint64, [C.c_void_p]),
    "rk_gzip_plan": (C.c_int64, [C.c_void_p, C.c_uint64]),
    "rk_gzip_calls": (C.c_int64, [C.c_void_p]),
    "rk_gzip_release_device": (None, [C.c_void_p]),
    "rk_gzip_stretch_bytes": (C.c_uint64, [C.c_void_p]),
    "rk_fastq_slot_reserve_gzip": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rk_fastq_slot_load_gzip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rk_bgzf_file_bytes": (C.c_uint64, [C.c_void_p]),
    # packed reads (`rkmh pack`, -F): include/rkmh_amd.h "PACKED READS"
    "rk_packed_encode": (C.c_int64, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "rk_packed_decode": (None, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rk_classify_batch_device_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.c_uint32, C.c_void_p]),
    "rk_count_batch_device_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.c_uint32, C.c_void_p]),
    "rk_packed_slot_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_packed_slot_destroy": (None, [C.c_void_p]),
    "rk_packed_slot_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rk_packed_slot_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rk_packed_filter_records_bound": (C.c_uint64, [C.c_void_p]),
    "rk_packed_filter_records": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64]),
    "rk_fastq_slot_create2": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
    "rk_fastq_slot_set_filter_output": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rk_fastq_slot_spans_base": (C.c_void_p, [C.c_void_p]),
    "rk_counter_create_compact": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rk_counter_compact_entries": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "rk_counter_entries": (C.c_uint64, [C.c_void_p]),
    "rk_counter_is_compact": (C.c_int, [C.c_void_p]),
    "rk_min_num_bound": (C.c_int, [C.c_void_p]),
    "rk_count_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64, C.c_void_p]),
    "rk_count_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rk_classify_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64, _i32p]),
    "rk_classify_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rk_classify_batch_device_all": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rk_call": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int, _u8p, _u64p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.POINTER(CallRecord)), C.POINTER(C.c_int64)]),
    "rk_format_stream_line": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rk_parse_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.POINTER(SeqSet)]),
    "rk_seqset_free": (None, [C.POINTER(SeqSet)]),
    "rk_pool_trim": (None, []),
    "rk_reader_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "rk_reader_next": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(SeqSet)]),
    "rk_reader_set_options": (None, [C.c_void_p, C.c_int]),
    "rk_reader_close": (None, [C.c_void_p]),
    "rk_reader_open_at": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_reader_open_range": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_reader_strict": (C.c_int, [C.c_void_p]),
    "rk_fastq_slot_create": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_fastq_slot_text": (C.c_void_p, [C.c_void_p]),
    "rk_fastq_slot_classify": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "rk_fastq_slot_destroy": (None, [C.c_void_p]),
    "rk_fastq_slot_submit": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rk_fastq_slot_finish": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rk_line_parts_create": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint64), C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rk_line_parts_destroy": (None, [C.c_void_p]),
    "rk_fastq_stream_lines_bound": (C.c_uint64, [C.c_void_p, C.c_void_p]),
    "rk_fastq_stream_lines": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "rk_fastq_filter_records_bound": (C.c_uint64, [C.c_void_p]),
    "rk_fastq_filter_records": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64]),
    "rk_fasta_load_create": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_fasta_load_put": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "rk_fasta_load_finish": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "rk_fasta_load_get_bases": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rk_set_references_fasta": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_uint64]),
    "rk_fasta_load_destroy": (None, [C.c_void_p]),
    "rk_fastq_slot_count": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "rk_fastq_cut": (C.c_int64, [C.c_void_p, C.c_uint64]),
    "rk_synth_reads": (C.c_int, [_u8p, _u64p, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _u8p, C.c_int]),
    "rk_compare_sketches": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_int, _u64p, _i32p, C.c_int, C.c_int, _i32p]),
    "rk_compare_sketches_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rk_merge_sketches": (C.c_int, [_u64p, _i32p, C.c_int, C.c_int, C.c_int, _u64p, _i32p]),
    "rk_mash_distance": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rk_scaled_max_hash": (C.c_int, [C.c_uint64, C.POINTER(C.c_uint64)]),
    "rk_sketch_scaled_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64, C.POINTER(C.c_int), C.c_int, C.c_uint64, C.POINTER(_u64p), _u64p]),
    "rk_compare_scaled": (C.c_int, [C.c_void_p, _u64p, _u64p, C.c_int, _u64p, _u64p, C.c_int, C.c_int, _i32p]),
    "rk_compare_scaled_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64,
                                           C.c_int, C.c_void_p, C.c_void_p]),
    "rk_merge_scaled": (C.c_int, [_u64p, _u64p, C.c_int, C.c_uint64, C.POINTER(_u64p), C.POINTER(C.c_uint64)]),
    "rk_scaled_distance": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rk_gather_scaled": (C.c_int, [C.c_void_p, _u64p, C.c_uint64, _u64p, _u64p, C.c_int, C.c_int, C.c_int, _i32p, _ip]),
    "rk_gather_scaled_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_int,
                                          C.c_void_p, _ip, C.c_void_p]),
    "rk_gather_scaled_host": (C.c_int, [_u64p, C.c_uint64, _u64p, _u64p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _ip]),
    "rk_sketch_scaled_abund_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64, C.POINTER(C.c_int), C.c_int, C.c_uint64, C.POINTER(_u64p),
                                               C.POINTER(_u32p), _u64p]),
    "rk_merge_scaled_abund": (C.c_int, [_u64p, _u32p, _u64p, C.c_int, C.c_uint64, C.POINTER(_u64p), C.POINTER(_u32p), C.POINTER(C.c_uint64)]),
    "rk_gather_scaled_abund": (C.c_int, [C.c_void_p, _u64p, _u32p, C.c_uint64, _u64p, _u64p, C.c_int, C.c_int, C.c_int, _i32p, _u64p, _ip]),
    "rk_gather_scaled_abund_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p, _ip, C.c_void_p]),
    "rk_gather_scaled_abund_host": (C.c_int, [_u64p, _u32p, C.c_uint64, _u64p, _u64p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _u64p, _ip]),
    "rk_compare_scaled_abund": (C.c_int, [C.c_void_p, _u64p, _u32p, _u64p, C.c_int, _u64p, _u32p, _u64p, C.c_int, C.c_int, _u64p]),
    "rk_compare_scaled_abund_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    "rk_abund_row_sums": (C.c_int, [C.c_void_p, _u32p, _u64p, C.c_int, _u64p]),
    "rk_abund_row_sums_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rk_compare_scaled_abund_host": (C.c_int, [_u64p, _u32p, _u64p, C.c_int, _u64p, _u32p, _u64p, C.c_int, C.c_int, _u64p]),
    "rk_abund_row_sums_host": (C.c_int, [_u32p, _u64p, C.c_int, _u64p]),
    "rk_angular_similarity": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rk_scaled_index_create": (C.c_int, [C.c_void_p, _u64p, _u64p, C.c_int64, C.POINTER(C.c_void_p)]),
    "rk_scaled_index_create_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rk_scaled_index_destroy": (None, [C.c_void_p]),
    "rk_scaled_index_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rk_search_scaled": (C.c_int, [C.c_void_p, C.c_void_p, _u64p, _u64p, C.c_int64, C.c_int, _i32p, C.POINTER(_i32p), C.POINTER(C.c_uint64)]),
    "rk_search_scaled_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
    "rk_search_scaled_host": (C.c_int, [_u64p, _u64p, C.c_int64, _u64p, _u64p, C.c_int64, C.c_int, _i32p, C.c_int, C.POINTER(_i32p),
                                        C.POINTER(C.c_uint64)]),
    "rk_search_min_count": (C.c_int, [C.c_double, C.c_uint64, C.POINTER(C.c_int32)]),
    "rk_multigather_scaled": (C.c_int, [C.c_void_p, C.c_void_p, _u64p, _u32p, _u64p, C.c_int64, C.c_int, C.c_int, C.POINTER(_i32p), C.POINTER(_u64p), _u64p,
                                        C.POINTER(C.c_uint64)]),
    "rk_multigather_scaled_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "rk_multigather_scaled_host": (C.c_int, [_u64p, _u64p, C.c_int64, _u64p, _u32p, _u64p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(_i32p),
                                             C.POINTER(_u64p), _u64p, C.POINTER(C.c_uint64)]),
    # cluster: include/rkmh_amd.h "CLUSTER"
    "rk_cluster_hits_host": (C.c_int, [_i32p, C.c_uint64, _u64p, C.c_int64, C.c_int, C.c_uint32, _i32p]),
    "rk_cluster_hits": (C.c_int, [C.c_void_p, _i32p, C.c_uint64, _u64p, C.c_int64, C.c_int, C.c_uint32, _i32p]),
    "rk_cluster_hits_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p,
                                         C.POINTER(C.c_uint32), C.c_void_p]),
    "rk_cluster_scaled": (C.c_int, [C.c_void_p, C.c_void_p, _u64p, _u64p, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_uint64, _i32p]),
    "rk_cluster_scaled_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_uint64,
                                           C.c_void_p, C.c_void_p]),
    "rk_cluster_members": (C.c_int, [_i32p, _u64p, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p, _i32p]),
    # the sample accumulator: include/rkmh_amd.h "SAMPLE SKETCHES"
    "rk_sample_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_sample_destroy": (None, [C.c_void_p]),
    "rk_sample_reset": (C.c_int, [C.c_void_p]),
    "rk_sample_add_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64]),
    "rk_sample_add_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rk_sample_add_sketch": (C.c_int, [C.c_void_p, _u64p, _u32p, C.c_uint64]),
    "rk_fastq_slot_sample": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "rk_sample_finish": (C.c_int, [C.c_void_p, C.POINTER(_u64p), C.POINTER(_u32p), C.POINTER(C.c_uint64)]),
    "rk_sample_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "rk_sample_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    # bottom samples: include/rkmh_amd.h "BOTTOM SAMPLES"
    "rk_sample_create_bottom": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rk_sample_finish_bottom": (C.c_int, [C.c_void_p, _u64p, _i32p]),
    "rk_sample_bottom_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "rk_bottom_cut": (C.c_int, [C.c_void_p, _u64p, _u32p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rk_bottom_emit": (C.c_int, [_u64p, _u32p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, _u64p, _i32p]),
    # screen: include/rkmh_amd.h "SCREEN"
    "rk_screen_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, _u64p, _u64p, C.c_int64, C.POINTER(C.c_void_p)]),
    "rk_screen_destroy": (None, [C.c_void_p]),
    "rk_screen_reset": (C.c_int, [C.c_void_p]),
    "rk_screen_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rk_screen_add_batch": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_int64]),
    "rk_screen_add_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rk_fastq_slot_screen": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "rk_screen_add_counts": (C.c_int, [C.c_void_p, _u64p, _u32p, C.c_uint64]),
    "rk_screen_rows": (C.c_int, [C.c_void_p, C.c_uint64, _u32p]),
    "rk_screen_rows_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rk_screen_counts": (C.c_int, [C.c_void_p, C.POINTER(_u64p), C.POINTER(_u64p), C.POINTER(C.c_uint64)]),
    "rk_screen_rows_host": (C.c_int, [_u64p, _u64p, C.c_int64, _u64p, _u64p, C.c_uint64, C.c_uint64, _u32p]),
    "rk_screen_identity": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
}


def _preload_torch_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (same SONAME as /opt/rocm's).
    If librkmh_amd.so pulled in the system copy first, a later `import torch` would bring a second runtime
    that finds no GPU.  So when torch is installed, its runtime is loaded first and the library binds to it."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library():
    """Loads librkmh_amd.so (built in-tree by `make` / __graft_entry__.build()). No fallback."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise RkmhError("%s is missing: build it with `make` (hipcc --offload-arch=gfx950). "
                            "rkmh_amd has no CPU fallback." % path)
        _preload_torch_hip_runtime()
        lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)  # AttributeError if the ABI drifted
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def _chk(rc):
    if rc != 0:
        cls = NeedFullDepthMap if rc == -7 else RkmhError
        e = cls("rkmh_amd error %d: %s" % (rc, load_library().rk_last_error().decode()))
        e.code = rc
        raise e


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _ks(ks):
    if np.isscalar(ks):
        ks = [ks]
    return np.ascontiguousarray(ks, dtype=np.int32)


def _padded(bases):
    """uint8 copy with >= 8 readable bytes past the end (device staging reads aligned dwords)."""
    b = np.zeros(len(bases) + 16, dtype=np.uint8)
    b[: len(bases)] = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else bases
    return b


def pack(seqs):
    """list[bytes] -> (uint8 bases (padded), uint64 offsets[n+1])"""
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return _padded(b"".join(seqs)), offs


def _seqset_to_py(ss):
    n = ss.nseq
    offs = np.ctypeslib.as_array(ss.offsets, shape=(n + 1,)).copy()
    nb = int(offs[-1])
    bases = np.zeros(nb + 16, dtype=np.uint8)
    if nb:
        bases[:nb] = np.ctypeslib.as_array(ss.bases, shape=(nb,))
    noffs = np.ctypeslib.as_array(ss.name_offsets, shape=(n + 1,)).copy()
    names_raw = (C.c_char * int(noffs[-1])).from_address(C.cast(ss.names, C.c_void_p).value).raw if n else b""
    names = [names_raw[int(noffs[i]): int(noffs[i + 1]) - 1] for i in range(n)]
    quals = None
    if ss.quals:
        q = (C.c_char * nb).from_address(C.cast(ss.quals, C.c_void_p).value).raw if nb else b""   # (string_at takes a C int: 2 GB at most)
        quals = [q[int(offs[i]): int(offs[i + 1])] for i in range(n)]
    return {"bases": bases, "offsets": offs, "names": names, "quals": quals, "nseq": n}


def _pinned_block(nbytes):
    """A ctypes byte array over rk_host_alloc memory that frees it when the LAST reference to the array goes away: numpy views made
    with np.frombuffer keep the ctypes object alive through their .base chain, so the page-locked memory lives exactly as long as
    any view of it (the DMA engine may still be reading or writing it until then)."""
    import weakref
    lib = load_library()
    ptr = C.c_void_p()
    _chk(lib.rk_host_alloc(max(nbytes, 1), C.byref(ptr)))
    buf = (C.c_uint8 * max(nbytes, 1)).from_address(ptr.value)
    weakref.finalize(buf, lib.rk_host_free, C.c_void_p(ptr.value))
    return buf


class PinnedArray:
    """A numpy array in page-locked host memory from rk_host_alloc: the host entry points read and write such buffers by DMA where
    they lie.  The memory belongs to `.array` (and to every view of it): it is freed when the last of them is collected, not when
    this wrapper is."""

    def __init__(self, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        buf = _pinned_block(nbytes)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def pinned_array(shape, dtype):
    return PinnedArray(shape, dtype)


def parse_files(paths):
    """parse_fastas (rkmh.cpp:238-292): FASTA/FASTQ(.gz) files -> dict(bases, offsets, names, quals)."""
    lib = load_library()
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    ss = SeqSet()
    _chk(lib.rk_parse_files(arr, len(paths), C.byref(ss)))
    try:
        return _seqset_to_py(ss)
    finally:
        lib.rk_seqset_free(C.byref(ss))


class Reader:
    """Streaming FASTA/FASTQ(.gz) reader (batches ready for Context.classify)."""

    def __init__(self, path, keep_quals=True):
        self._lib = load_library()
        self._h = C.c_void_p()
        _chk(self._lib.rk_reader_open(os.fsencode(path), C.byref(self._h)))
        if not keep_quals:
            self._lib.rk_reader_set_options(self._h, 1)

    def next_batch(self, max_records=1 << 20, max_bases=1 << 28):
        ss = SeqSet()
        _chk(self._lib.rk_reader_next(self._h, max_records, max_bases, C.byref(ss)))
        try:
            return _seqset_to_py(ss) if ss.nseq else None
        finally:
            self._lib.rk_seqset_free(C.byref(ss))

    def close(self):
        if self._h:
            self._lib.rk_reader_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pool_trim():
    """Returns the parser's parked batch buffers (up to 1.5 GB) to the system (rk_pool_trim)."""
    load_library().rk_pool_trim()


def parse_file_range(path, lo, hi):
    """The records that START in bytes [lo, hi) of a regular uncompressed FASTQ file (rk_reader_open_range): how each rank of a
    multi-process run reads only its own part of the reads.  Returns the same dict as parse_files plus "strict": False means the
    text is not four lines per record, the range boundaries cannot be trusted and the caller must parse the whole file instead.
    Raises RkmhError for input that cannot be split at all (gzip, FASTA, STDIN)."""
    lib = load_library()
    h = C.c_void_p()
    _chk(lib.rk_reader_open_range(os.fsencode(path), int(lo), int(hi), C.byref(h)))
    parts = []
    try:
        while True:
            ss = SeqSet()
            _chk(lib.rk_reader_next(h, 1 << 22, 1 << 30, C.byref(ss)))
            n = ss.nseq
            if n:
                parts.append(_seqset_to_py(ss))
            lib.rk_seqset_free(C.byref(ss))
            if n == 0:
                break
        strict = bool(lib.rk_reader_strict(h))
    finally:
        lib.rk_reader_close(h)
    if not parts:
        return {"bases": np.zeros(16, np.uint8), "offsets": np.zeros(1, np.uint64), "names": [], "quals": [], "nseq": 0, "strict": strict}
    out = parts[0]
    for p in parts[1:]:
        nb = int(out["offsets"][-1])
        out["bases"] = np.concatenate([out["bases"][:nb], p["bases"]])
        out["offsets"] = np.concatenate([out["offsets"], p["offsets"][1:] + np.uint64(nb)])
        out["names"] += p["names"]
        out["quals"] = None if out["quals"] is None or p["quals"] is None else out["quals"] + p["quals"]
        out["nseq"] += p["nseq"]
    out["strict"] = strict
    return out


def format_stream_line(ref_name, read_name, max_shared, diff, min_num, sketch_size, min_matches=-1, min_diff=0):
    lib = load_library()
    cap = len(ref_name) + len(read_name) + 128
    buf = C.create_string_buffer(cap)
    n = lib.rk_format_stream_line(buf, cap, ref_name, read_name, max_shared, diff, min_num, sketch_size,
                                  min_matches, min_diff)
    if n < 0:
        _chk(n)
    return buf.raw[:n]


def device_props(device=0) -> dict:
    """{'compute_units', 'clock_khz', 'l2_bytes', 'hbm_bytes'} of a GPU (hipGetDeviceProperties)."""
    lib = load_library()
    cu, khz, l2, hbm = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    _chk(lib.rk_device_props(device, C.byref(cu), C.byref(khz), C.byref(l2), C.byref(hbm)))
    return {"compute_units": cu.value, "clock_khz": khz.value, "l2_bytes": l2.value, "hbm_bytes": hbm.value}


class FastqResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("nrec", C.c_int64), ("out4", C.POINTER(C.c_int32)), ("name_off", C.POINTER(C.c_uint32)),
                ("name_len", C.POINTER(C.c_uint32)), ("seq_off", C.POINTER(C.c_uint32)), ("seq_len", C.POINTER(C.c_uint32)),
                ("qual_off", C.POINTER(C.c_uint32))]


class FastaIndex(C.Structure):
    _fields_ = [("status", C.c_int32), ("nseq", C.c_int64), ("offsets", C.POINTER(C.c_uint64)), ("names", C.c_void_p),
                ("name_offsets", C.POINTER(C.c_uint64))]


class FastaLoad:
    """Reference FASTA text stripped on the device (rk_fasta_load_*): put() the raw text of the -r files block by block through a
    FastqSlot's page-locked buffer, finish() returns (status, names, offsets) -- status != 0: parse on the host --, then
    set_references() sketches the packed bases where they lie."""

    def __init__(self, ctx, text_bytes):
        self._lib = load_library()
        self._ctx = ctx
        self._h = C.c_void_p()
        self.text_bytes = text_bytes
        _chk(self._lib.rk_fasta_load_create(ctx._h, text_bytes, C.byref(self._h)))

    def put(self, slot, offset, text: bytes):
        if len(text) > slot.max_bytes:
            raise ValueError("block larger than the slot")
        C.memmove(self._lib.rk_fastq_slot_text(slot._h), text, len(text))
        _chk(self._lib.rk_fasta_load_put(self._h, slot._h, offset, len(text)))

    def put_raw(self, slot, offset, nbytes):
        """The first nbytes of the slot's text_buffer() (filled by the caller) become text[offset ..)."""
        _chk(self._lib.rk_fasta_load_put(self._h, slot._h, offset, nbytes))

    def finish(self, total_bytes=None):
        res = FastaIndex()
        _chk(self._lib.rk_fasta_load_finish(self._h, self.text_bytes if total_bytes is None else total_bytes, C.byref(res)))
        if res.status != 0:
            return int(res.status), [], np.zeros(1, np.uint64)
        n = int(res.nseq)
        offs = np.ctypeslib.as_array(res.offsets, shape=(n + 1,)).copy()
        noff = np.ctypeslib.as_array(res.name_offsets, shape=(n + 1,))
        blob = C.string_at(res.names, int(noff[n]))
        names = [blob[int(noff[i]): int(noff[i + 1]) - 1] for i in range(n)]
        self._total = int(offs[n])
        return 0, names, offs

    def bases(self):
        """The packed bases on the host (rk_fasta_load_get_bases), as the text spells them."""
        out = np.zeros(self._total + 16, dtype=np.uint8)
        _chk(self._lib.rk_fasta_load_get_bases(self._h, out.ctypes.data_as(C.c_void_p)))
        return out[: self._total]

    def set_references(self, ks, sketch_size, max_samples=-1, counter_slots=0):
        arr = (C.c_int * len(ks))(*ks)
        _chk(self._lib.rk_set_references_fasta(self._ctx._h, self._h, arr, len(ks), sketch_size, max_samples, counter_slots))
        self._ctx.sketch_size, self._ctx.ks = sketch_size, _ks(ks)

    def destroy(self):
        if self._h:
            self._lib.rk_fasta_load_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def fastq_cut(text: bytes) -> int:
    """Offset of the last record start in text[1:] under the four-line rule, or -1 (rk_fastq_cut)."""
    b = (C.c_char * len(text)).from_buffer_copy(text)
    return int(load_library().rk_fastq_cut(C.cast(b, C.c_void_p), len(text)))


class LineParts:
    """What does not depend on the read in a stream / classify line (rk_line_parts): reference names with their tab, the eight tails."""

    def __init__(self, ref_names, sketch_size, min_matches, min_diff):
        self._lib = load_library()
        self._h = C.c_void_p()
        blob = b"".join(bytes(n) + b"\0" for n in ref_names)
        offs = np.zeros(len(ref_names) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(n) + 1 for n in ref_names])
        _chk(self._lib.rk_line_parts_create(blob, offs.ctypes.data_as(C.POINTER(C.c_uint64)), len(ref_names), sketch_size, min_matches, min_diff,
                                            C.byref(self._h)))

    def destroy(self):
        if self._h:
            self._lib.rk_line_parts_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class FastqSlot:
    """One block of raw FASTQ text in flight (rk_fastq_slot_*): the text is split into records, checked, packed and classified on the device."""

    def __init__(self, ctx, max_bytes=1 << 26, device_text=False):
        """device_text: RK_SLOT_DEVICE_TEXT -- the block's text stays on the device (blocks come from load_bgzf), only rows and the
        packed names (or, after set_filter_output, the records filter prints) come back."""
        self._lib = load_library()
        self._h = C.c_void_p()
        self.max_bytes = max_bytes
        self.device_text = bool(device_text)
        _chk(self._lib.rk_fastq_slot_create2(ctx._h, max_bytes, 1 if device_text else 0, C.byref(self._h)))

    def set_filter_output(self, min_matches, min_diff):
        _chk(self._lib.rk_fastq_slot_set_filter_output(self._h, min_matches, min_diff))

    def classify(self, text: bytes):
        """Returns (status, rows [n,4] int32, names [n] bytes, seqs [n] bytes); status != 0: the block must be parsed on the host."""
        self.submit(text)
        return self.finish()

    def count(self, text: bytes, counter):
        """Pass 1 of -M on a block (rk_fastq_slot_count): returns (status, records); status != 0: nothing was counted."""
        n = len(text)
        if n > self.max_bytes:
            raise ValueError("block larger than the slot")
        C.memmove(self._lib.rk_fastq_slot_text(self._h), text, n)
        st, nrec = C.c_int32(), C.c_int64()
        _chk(self._lib.rk_fastq_slot_count(self._h, n, counter._h, C.byref(st), C.byref(nrec)))
        return st.value, nrec.value

    def sample(self, text, sample):
        """A block into a Sample (rk_fastq_slot_sample): returns (status, records); status != 0: nothing of it was added.  text: bytes,
        or -- for a slot whose block was named with set_source or loaded on the device -- the number of bytes."""
        if isinstance(text, (bytes, bytearray)):
            n = len(text)
            if n > self.max_bytes:
                raise ValueError("block larger than the slot")
            if self.device_text:
                raise ValueError("a device-text slot takes its block from set_source or load_bgzf: pass the number of bytes")
            C.memmove(self._lib.rk_fastq_slot_text(self._h), bytes(text), n)
        else:
            n = int(text)
        st, nrec = C.c_int32(), C.c_int64()
        _chk(self._lib.rk_fastq_slot_sample(self._h, n, sample._h, C.byref(st), C.byref(nrec)))
        return st.value, nrec.value

    def screen(self, text, screen):
        """A block into a Screen (rk_fastq_slot_screen): as sample() -> (status, records); status != 0: nothing of it was added."""
        if isinstance(text, (bytes, bytearray)):
            n = len(text)
            if n > self.max_bytes:
                raise ValueError("block larger than the slot")
            if self.device_text:
                raise ValueError("a device-text slot takes its block from set_source or load_bgzf: pass the number of bytes")
            C.memmove(self._lib.rk_fastq_slot_text(self._h), bytes(text), n)
        else:
            n = int(text)
        st, nrec = C.c_int32(), C.c_int64()
        _chk(self._lib.rk_fastq_slot_screen(self._h, n, screen._h, C.byref(st), C.byref(nrec)))
        return st.value, nrec.value

    def set_source(self, address):
        """rk_fastq_slot_set_source: the next block is read from caller memory at `address` (valid until the block's call has returned)."""
        _chk(self._lib.rk_fastq_slot_set_source(self._h, C.c_void_p(address)))

    # -- the zero-copy forms the one-process-per-GPU front end uses (rkmh_amd/cli.py): the caller reads file bytes straight into the
    # slot's page-locked buffer and the output text is formatted in C from the result where it lies
    def text_buffer(self):
        """The slot's page-locked text buffer as a writable ctypes array (max_bytes + 64 bytes): os.preadv() into it."""
        return (C.c_char * (self.max_bytes + 64)).from_address(self._lib.rk_fastq_slot_text(self._h))

    def load_bgzf(self, bz, b0, b1):
        """Members [b0, b1) of a Bgzf file inflated on the device into this slot (rk_fastq_slot_load_bgzf) -> (status, nbytes, text
        offset); status 1: take the host route.  Follow with classify_raw(nbytes) / count_raw(nbytes, counter)."""
        n, off = C.c_uint64(), C.c_uint64()
        rc = self._lib.rk_fastq_slot_load_bgzf(self._h, bz._h, b0, b1, C.byref(n), C.byref(off))
        if rc < 0:
            _chk(rc)
        return rc, int(n.value), int(off.value)

    def load_gzip(self, gz, call):
        """Stretch number `call` of a Gzip file (an ordinary one-stream .gz) inflated on the device into this slot
        (rk_fastq_slot_load_gzip) -> (status, nbytes, text offset); status 1: the sequential reader continues from the text offset."""
        n, off = C.c_uint64(), C.c_uint64()
        rc = self._lib.rk_fastq_slot_load_gzip(self._h, gz._h, call, C.byref(n), C.byref(off))
        if rc < 0:
            _chk(rc)
        return rc, int(n.value), int(off.value)

    def classify_raw(self, nbytes):
        """rk_fastq_slot_classify on the first nbytes of text_buffer(); returns the FastqResult structure (valid until the next call)."""
        res = FastqResult()
        _chk(self._lib.rk_fastq_slot_classify(self._h, nbytes, C.byref(res)))
        return res

    def count_raw(self, nbytes, counter):
        st, nrec = C.c_int32(), C.c_int64()
        _chk(self._lib.rk_fastq_slot_count(self._h, nbytes, counter._h, C.byref(st), C.byref(nrec)))
        return st.value, nrec.value

    def _out_buffer(self, cap):
        # one growing buffer per slot (a slot serves one thread): no allocation or zero-fill per block
        if getattr(self, "_obuf", None) is None or len(self._obuf) < cap:
            self._obuf = bytearray(cap + cap // 8)
        return (C.c_char * len(self._obuf)).from_buffer(self._obuf)

    def stream_lines(self, parts, res):
        """The stream / classify lines of a classified block (rk_fastq_stream_lines), as bytes."""
        cap = int(self._lib.rk_fastq_stream_lines_bound(parts._h, C.byref(res)))
        buf = self._out_buffer(cap)
        n = self._lib.rk_fastq_stream_lines(parts._h, C.byref(res), self._lib.rk_fastq_slot_spans_base(self._h), buf, len(self._obuf))
        del buf
        if n < 0:
            _chk(int(n))
        return bytes(memoryview(self._obuf)[:n])

    def filter_records(self, res, min_matches, min_diff):
        """filter's records of a classified block (rk_fastq_filter_records), as bytes."""
        cap = int(self._lib.rk_fastq_filter_records_bound(C.byref(res)))
        buf = self._out_buffer(cap)
        n = self._lib.rk_fastq_filter_records(C.byref(res), self._lib.rk_fastq_slot_spans_base(self._h), min_matches, min_diff, buf, len(self._obuf))
        del buf
        if n < 0:
            _chk(int(n))
        return bytes(memoryview(self._obuf)[:n])

    def submit(self, text: bytes):
        """First half (rk_fastq_slot_submit): the upload and the splitting kernels are enqueued; returns at once."""
        n = len(text)
        if n > self.max_bytes:
            raise ValueError("block larger than the slot")
        C.memmove(self._lib.rk_fastq_slot_text(self._h), text, n)
        self._text = text
        _chk(self._lib.rk_fastq_slot_submit(self._h, n))

    def finish(self):
        """Second half (rk_fastq_slot_finish): waits, classifies, collects; same return value as classify()."""
        text = self._text
        res = FastqResult()
        _chk(self._lib.rk_fastq_slot_finish(self._h, C.byref(res)))
        if res.status != 0 or res.nrec == 0:
            return int(res.status), np.zeros((0, 4), np.int32), [], []
        m = int(res.nrec)
        rows = np.ctypeslib.as_array(res.out4, shape=(m, 4)).copy()
        no = np.ctypeslib.as_array(res.name_off, shape=(m,)); nl = np.ctypeslib.as_array(res.name_len, shape=(m,))
        so = np.ctypeslib.as_array(res.seq_off, shape=(m,)); sl = np.ctypeslib.as_array(res.seq_len, shape=(m,))
        names = [text[int(no[i]): int(no[i]) + int(nl[i])] for i in range(m)]
        seqs = [text[int(so[i]): int(so[i]) + int(sl[i])] for i in range(m)]
        qo = np.ctypeslib.as_array(res.qual_off, shape=(m,))
        self.last_quals = [text[int(qo[i]): int(qo[i]) + int(sl[i])] for i in range(m)]  # the quality strings of the block just finished
        return 0, rows, names, seqs

    def destroy(self):
        if self._h:
            self._lib.rk_fastq_slot_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Gzip:
    """An ordinary gzip file -- one deflate stream -- that the device inflates stretch after stretch (rk_gzip_*, rk_gunzip.hip).
    Gzip.open returns None for anything that is not a gzip file."""

    def __init__(self, handle):
        self._lib = load_library()
        self._h = handle

    @staticmethod
    def open(path):
        lib = load_library()
        h = C.c_void_p()
        rc = lib.rk_gzip_open(os.fsencode(path), C.byref(h))
        if rc != 0:
            return None
        return Gzip(h)

    def first_byte(self):
        return int(self._lib.rk_gzip_first_byte(self._h))

    @property
    def text_bytes_hint(self):
        return int(self._lib.rk_gzip_text_bytes_hint(self._h))

    def plan(self, slot_bytes):
        """how many load_gzip calls the file takes with slots of slot_bytes; rewinds the stream"""
        n = int(self._lib.rk_gzip_plan(self._h, slot_bytes))
        if n < 0:
            _chk(-1)
        return n

    def release_device(self):
        self._lib.rk_gzip_release_device(self._h)

    def close(self):
        if self._h:
            self._lib.rk_gzip_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bgzf:
    """A BGZF (bgzip) file whose members any number of threads may inflate (rk_bgzf_*): the compressed form of the device FASTQ
    front end's input.  Bgzf.open returns None for anything that is not BGZF."""

    def __init__(self, handle):
        self._lib = load_library()
        self._h = handle

    @staticmethod
    def open(path):
        lib = load_library()
        h = C.c_void_p()
        rc = lib.rk_bgzf_open(os.fsencode(path), C.byref(h))
        if rc == -1:         # RK_ERR_ARG: not BGZF
            return None
        _chk(rc)
        return Bgzf(h)

    @property
    def members(self):
        return int(self._lib.rk_bgzf_members(self._h))

    @property
    def text_bytes(self):
        return int(self._lib.rk_bgzf_text_bytes(self._h))

    def text_offset(self, member):
        return int(self._lib.rk_bgzf_text_offset(self._h, member))

    def first_byte(self):
        return int(self._lib.rk_bgzf_first_byte(self._h))

    def plan(self, target_bytes):
        """first members of the jobs of about target_bytes of text each, and the member count last"""
        cap = self.members + 2
        first = (C.c_int64 * cap)()
        n = int(self._lib.rk_bgzf_plan(self._h, target_bytes, first, cap))
        if n < 0:
            _chk(n)
        return [int(first[i]) for i in range(n + 1)]

    def fastq_records(self, b0, b1, dst, cap):
        """the whole FASTQ records that start in members [b0, b1) -> (status, bytes written to dst, their offset in the text);
        status 1: the text does not begin with '@'.  dst: address or ctypes buffer of cap bytes."""
        n, off = C.c_uint64(), C.c_uint64()
        rc = self._lib.rk_bgzf_fastq_records(self._h, b0, b1, dst, cap, C.byref(n), C.byref(off))
        if rc < 0:
            _chk(rc)
        return rc, int(n.value), int(off.value)

    def close(self):
        if self._h:
            self._lib.rk_bgzf_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Counter:
    """HASHTCounter (rkmh.cpp:739): int32 table in HBM, slot = key % slots."""

    def __init__(self, ctx, slots=None, device_ptr=None, compact=False):
        """compact=True: the compact depth map of rk_counter_create_compact (only the slots of index keys; needs the references set
        and min_num bound 0); device_ptr then names zeroed memory of Counter.compact_entries(ctx, slots) int32, or None."""
        self._lib = load_library()
        self._ctx = ctx
        self._h = C.c_void_p()
        if compact:
            _chk(self._lib.rk_counter_create_compact(ctx._h, slots, C.c_void_p(device_ptr) if device_ptr is not None else None, C.byref(self._h)))
        elif device_ptr is not None:
            _chk(self._lib.rk_counter_wrap(ctx._h, C.c_void_p(device_ptr), slots, C.byref(self._h)))
        else:
            _chk(self._lib.rk_counter_create(ctx._h, slots, C.byref(self._h)))

    def increment(self, key):
        _chk(self._lib.rk_counter_increment(self._h, int(key)))

    def get(self, key):
        v = C.c_int32()
        _chk(self._lib.rk_counter_get(self._h, int(key), C.byref(v)))
        return v.value

    def clear(self):
        _chk(self._lib.rk_counter_clear(self._h))

    def add(self, other):
        """self += other (tables of equal size, possibly on two devices of this process): the reduce step of a multi-device -M run."""
        _chk(self._lib.rk_counter_add(self._h, other._h))

    def copy_from(self, other):
        """self = other (the broadcast step)."""
        _chk(self._lib.rk_counter_copy(self._h, other._h))

    def save(self, path, tag=None):
        """tag: bytes from Context.depth_map_tag (provenance of a read-depth map) or None for an untagged file."""
        if tag is None:
            _chk(self._lib.rk_counter_save(self._h, os.fsencode(path)))
        else:
            _chk(self._lib.rk_counter_save_tagged(self._h, os.fsencode(path), C.c_char_p(bytes(tag)), len(tag)))

    def load(self, path, tag=None):
        """Refuses (RkmhError) a file whose provenance tag differs from `tag` (tagged vs untagged included)."""
        if tag is None:
            _chk(self._lib.rk_counter_load(self._h, os.fsencode(path)))
        else:
            _chk(self._lib.rk_counter_load_tagged(self._h, os.fsencode(path), C.c_char_p(bytes(tag)), len(tag)))

    @staticmethod
    def compact_entries(ctx, slots):
        n = C.c_uint64()
        _chk(load_library().rk_counter_compact_entries(ctx._h, slots, C.byref(n)))
        return int(n.value)

    @property
    def slots(self):
        return int(self._lib.rk_counter_slots(self._h))

    @property
    def entries(self):
        return int(self._lib.rk_counter_entries(self._h))

    @property
    def compact(self):
        return bool(self._lib.rk_counter_is_compact(self._h))

    @property
    def device_ptr(self):
        return int(self._lib.rk_counter_device_ptr(self._h))

    def destroy(self):
        if self._h:
            self._lib.rk_counter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def parse_policy(spec=None, base=None):
    """rk_policy_parse: `spec` (presets default / mash / sourmash, or fold= / windows= / zero= / mask= / freqmax= / canon= / dedup= / seed=) applied onto `base`
    (default: the build's defaults).  Raises RkmhError on text it does not know."""
    lib = load_library()
    p = Policy()
    if base is None:
        lib.rk_default_policy(C.byref(p))
    else:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(Policy))
    if spec:
        _chk(lib.rk_policy_parse(spec.encode() if isinstance(spec, str) else spec, C.byref(p)))
    return p


def describe_policy(p):
    """rk_policy_describe: the canonical text of a policy, every key spelled out."""
    buf = C.create_string_buffer(160)
    n = load_library().rk_policy_describe(C.byref(p), buf, len(buf))
    if n < 0:
        _chk(n)
    return buf.value.decode()


def merge_sketches(sketches, lens, sketch_size=None, distinct=False):
    """rk_merge_sketches (host code, no GPU): the bottom sketch_size of the union of the rows of `sketches` (uint64 [n, sketch_size],
    the first lens[i] of row i are its values) -> (uint64 [sketch_size] zero padded, length).  distinct: each value once."""
    sketches = np.ascontiguousarray(sketches, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    if sketch_size is None:
        sketch_size = sketches.shape[1]
    n = len(lens)
    if sketches.size != n * sketch_size:
        raise ValueError("sketches must hold len(lens) rows of sketch_size values")
    out = np.zeros(max(sketch_size, 1), dtype=np.uint64)
    m = C.c_int32()
    _chk(load_library().rk_merge_sketches(_p(sketches, C.c_uint64), _p(lens, C.c_int32), n, sketch_size, 1 if distinct else 0,
                                          _p(out, C.c_uint64), C.byref(m)))
    return out[:sketch_size], int(m.value)


def mash_distance(common, denom, k):
    """rk_mash_distance (host code, no GPU): (jaccard, distance) from fields 2 and 3 of a compare_sketches row."""
    j, d = C.c_double(), C.c_double()
    _chk(load_library().rk_mash_distance(int(common), int(denom), int(k), C.byref(j), C.byref(d)))
    return j.value, d.value


def scaled_max_hash(scaled):
    """rk_scaled_max_hash (host code, no GPU): floor((2^64 - 1) / scaled); a scaled sketch keeps the hashes 0 < h <= max_hash."""
    v = C.c_uint64()
    _chk(load_library().rk_scaled_max_hash(C.c_uint64(int(scaled)), C.byref(v)))
    return int(v.value)


def _csr(values, offsets):
    values = np.ascontiguousarray(values, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) < 1 or int(offsets[-1]) > len(values) or int(offsets.max()) > len(values):
        raise ValueError("offsets run past the %d values" % len(values))
    return values, offsets


def merge_scaled(values, offsets, max_hash=(1 << 64) - 1):
    """rk_merge_scaled (host code, no GPU): the ascending distinct union of the CSR sketches (values, offsets[n + 1]) cut at
    max_hash -> uint64 array.  One sketch and a smaller max_hash: that sketch at a larger `scaled`."""
    values, offsets = _csr(values, offsets)
    out, n = _u64p(), C.c_uint64()
    lib = load_library()
    _chk(lib.rk_merge_scaled(_p(values, C.c_uint64), _p(offsets, C.c_uint64), len(offsets) - 1, C.c_uint64(int(max_hash)), C.byref(out), C.byref(n)))
    r = np.ctypeslib.as_array(out, shape=(max(int(n.value), 1),))[: int(n.value)].copy()
    lib.rk_free(out)
    return r


def scaled_distance(shared, la, lb, k):
    """rk_scaled_distance (host code, no GPU): (jaccard, distance) of two scaled sketches of la and lb values that share `shared`."""
    j, d = C.c_double(), C.c_double()
    _chk(load_library().rk_scaled_distance(int(shared), int(la), int(lb), int(k), C.byref(j), C.byref(d)))
    return j.value, d.value


RK_GATHER_BATCH = 16  # include/rkmh_amd.h: rounds of gather enqueued between two looks at the state


def _gather_args(q, r_values, r_offsets, max_rounds):
    q = np.ascontiguousarray(q, dtype=np.uint64)
    r_values, r_offsets = _csr(r_values, r_offsets)
    nref = len(r_offsets) - 1
    max_rounds = nref if max_rounds is None else int(max_rounds)
    return q, r_values, r_offsets, nref, max_rounds, np.zeros((max(min(max_rounds, nref), 0), 4), dtype=np.int32)


def gather_scaled_host(q, r_values, r_offsets, min_shared=1, max_rounds=None, threads=1):
    """rk_gather_scaled_host (host code, no GPU): the rows of Context.gather_scaled from the same loop on `threads` host threads."""
    q, r_values, r_offsets, nref, max_rounds, out = _gather_args(q, r_values, r_offsets, max_rounds)
    n = C.c_int(0)
    _chk(load_library().rk_gather_scaled_host(_p(q, C.c_uint64), len(q), _p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), nref, int(min_shared),
                                              max_rounds, int(threads), _p(out, C.c_int32), C.byref(n)))
    return out[: n.value].copy()


RK_SEARCH_REF_BLOCK = 8192  # include/rkmh_amd.h: references per workgroup of the search kernel


class ScaledIndexStats(C.Structure):
    """rk_scaled_index_stats_t (rkmh_amd.h, "SEARCH")"""
    _fields_ = [("struct_size", C.c_uint32), ("nref", C.c_uint32), ("npost", C.c_uint64), ("nkeys", C.c_uint64), ("longest_posting", C.c_uint32),
                ("reserved", C.c_uint32)]


def _q_min(q_min, nq):
    """the per-query thresholds: None, or int32 [nq]"""
    if q_min is None:
        return None
    q_min = np.ascontiguousarray(q_min, dtype=np.int32)
    if q_min.ndim != 1 or len(q_min) != nq:
        raise ValueError("%d thresholds for %d queries" % (q_min.size, nq))
    return q_min


def _hits(lib, out, n):
    """the malloc'd hits of a search -> int32 [n, 3] (query, reference, shared); releases them"""
    r = np.ctypeslib.as_array(out, shape=(max(n, 1) * 3,))[: n * 3].copy().reshape(n, 3)
    lib.rk_free(out)
    return r


def search_scaled_host(r_values, r_offsets, q_values, q_offsets, min_shared=1, q_min=None, threads=1):
    """rk_search_scaled_host (host code, no GPU): every pair of a CSR query sketch and a CSR reference sketch that shares at least
    max(min_shared, q_min[query]) values -> int32 [n, 3], rows (query, reference, shared) sorted by (query, reference)."""
    r_values, r_offsets = _csr(r_values, r_offsets)
    q_values, q_offsets = _csr(q_values, q_offsets)
    nq = len(q_offsets) - 1
    q_min = _q_min(q_min, nq)
    out, n = _i32p(), C.c_uint64()
    lib = load_library()
    _chk(lib.rk_search_scaled_host(_p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), len(r_offsets) - 1, _p(q_values, C.c_uint64),
                                   _p(q_offsets, C.c_uint64), nq, int(min_shared), None if q_min is None else _p(q_min, C.c_int32), int(threads),
                                   C.byref(out), C.byref(n)))
    return _hits(lib, out, int(n.value))


def search_min_count(min_containment, length):
    """rk_search_min_count (host code, no GPU): the smallest t with t / length >= min_containment, the count `rkmh manysearch
    --min-containment` asks of a query of `length` values (0 for an empty query)."""
    t = C.c_int32()
    _chk(load_library().rk_search_min_count(float(min_containment), C.c_uint64(int(length)), C.byref(t)))
    return int(t.value)


RK_CLUSTER_JACCARD, RK_CLUSTER_MAX_CONTAINMENT = 0, 1  # include/rkmh_amd.h "CLUSTER": the measure of a link


def _cluster_args(hits, lens):
    """the hits and lengths of a clustering, checked -> (int32 [nhits, 3], uint64 [n], labels int32 [n])"""
    hits = np.ascontiguousarray(hits, dtype=np.int32).reshape(-1, 3)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    if lens.ndim != 1:
        raise ValueError("lens is not one-dimensional")
    return hits, lens, np.zeros(len(lens), dtype=np.int32)


def cluster_hits_host(hits, lens, measure=RK_CLUSTER_JACCARD, min_ppm=0):
    """rk_cluster_hits_host (host code, no GPU): the single-linkage clusters of n sketches of the lengths `lens` under the hits (rows
    (query, reference, shared)) that link at `measure` and `min_ppm` parts per million -> int32 [n]: the smallest index of every
    sketch's cluster."""
    hits, lens, labels = _cluster_args(hits, lens)
    _chk(load_library().rk_cluster_hits_host(_p(hits, C.c_int32), C.c_uint64(len(hits)), _p(lens, C.c_uint64), len(lens), int(measure),
                                             C.c_uint32(int(min_ppm)), _p(labels, C.c_int32)))
    return labels


def cluster_members(labels, lens):
    """rk_cluster_members (host code, no GPU) -> (cl_off int32 [ncl + 1], members int32 [n], rep int32 [ncl]): the clusters ordered by
    their smallest member, members ascending; rep: the member with the largest length, among equal lengths the lowest index."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    if labels.ndim != 1 or lens.shape != labels.shape:
        raise ValueError("%d labels for %d lengths" % (labels.size, lens.size))
    n = len(labels)
    ncl = C.c_int64()
    cl_off, members, rep = np.zeros(n + 1, dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    _chk(load_library().rk_cluster_members(_p(labels, C.c_int32), _p(lens, C.c_uint64), n, C.byref(ncl), _p(cl_off, C.c_int32), _p(members, C.c_int32),
                                           _p(rep, C.c_int32)))
    return cl_off[: ncl.value + 1].copy(), members[:n], rep[: ncl.value].copy()


def _multigather_args(q_values, q_offsets, q_abund, max_rounds):
    """the query batch of a multigather, checked -> (values, offsets, abundances or None, nq, max_rounds, row_offsets uint64 [nq + 1])"""
    q_values, q_offsets = _csr(q_values, q_offsets)
    if q_abund is not None:
        q_abund = _abund(q_abund, q_values)
    nq = len(q_offsets) - 1
    max_rounds = 0x7fffffff if max_rounds is None else int(max_rounds)   # no reference is picked twice: as many rows as there are candidates
    return q_values, q_offsets, q_abund, nq, max_rounds, np.zeros(nq + 1, dtype=np.uint64)


def _multigather_rows(lib, out, wu, n, weighted):
    """the malloc'd answer of a multigather -> (int32 [n, 4], uint64 [n] or None); releases it"""
    rows = np.ctypeslib.as_array(out, shape=(max(n, 1) * 4,))[: n * 4].copy().reshape(n, 4)
    lib.rk_free(out)
    w = None
    if weighted:
        w = np.ctypeslib.as_array(wu, shape=(max(n, 1),))[:n].copy()
        lib.rk_free(wu)
    return rows, w


def multigather_scaled_host(r_values, r_offsets, q_values, q_offsets, q_abund=None, min_shared=1, max_rounds=None, threads=1):
    """rk_multigather_scaled_host (host code, no GPU): gather_scaled_host for every row of the CSR query batch, the queries shared among
    `threads` host threads -> (rows int32 [n, 4], row_offsets uint64 [nq + 1], wunique uint64 [n] or None): the rows of query i are
    rows[row_offsets[i]:row_offsets[i + 1]], in pick order."""
    r_values, r_offsets = _csr(r_values, r_offsets)
    q_values, q_offsets, q_abund, nq, max_rounds, ro = _multigather_args(q_values, q_offsets, q_abund, max_rounds)
    out, wu, n = _i32p(), _u64p(), C.c_uint64()
    lib = load_library()
    _chk(lib.rk_multigather_scaled_host(_p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), len(r_offsets) - 1, _p(q_values, C.c_uint64),
                                        None if q_abund is None else _p(q_abund, C.c_uint32), _p(q_offsets, C.c_uint64), nq, int(min_shared), max_rounds,
                                        int(threads), C.byref(out), C.byref(wu), _p(ro, C.c_uint64), C.byref(n)))
    rows, w = _multigather_rows(lib, out, wu, int(n.value), q_abund is not None)
    return rows, ro, w


class ScaledIndex:
    """rk_scaled_index: the resident inverted index of a collection of scaled sketches (Context.scaled_index)."""

    def __init__(self, ctx, handle):
        self._ctx, self._lib, self._h = ctx, ctx._lib, handle

    def close(self):
        if self._h:
            self._lib.rk_scaled_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        """-> dict(nref, npost, nkeys, longest_posting)"""
        s = ScaledIndexStats()
        s.struct_size = C.sizeof(ScaledIndexStats)
        _chk(self._lib.rk_scaled_index_stats(self._h, C.byref(s)))
        return dict(nref=int(s.nref), npost=int(s.npost), nkeys=int(s.nkeys), longest_posting=int(s.longest_posting))

    def search(self, q_values, q_offsets, min_shared=1, q_min=None):
        """rk_search_scaled: the CSR query sketches against the index -> int32 [n, 3], rows (query, reference, shared) of every pair
        that shares at least max(min_shared, q_min[query]) values, sorted by (query, reference)."""
        q_values, q_offsets = _csr(q_values, q_offsets)
        nq = len(q_offsets) - 1
        q_min = _q_min(q_min, nq)
        out, n = _i32p(), C.c_uint64()
        _chk(self._lib.rk_search_scaled(self._ctx._h, self._h, _p(q_values, C.c_uint64), _p(q_offsets, C.c_uint64), nq, int(min_shared),
                                        None if q_min is None else _p(q_min, C.c_int32), C.byref(out), C.byref(n)))
        return _hits(self._lib, out, int(n.value))

    def search_device(self, d_q_values_ptr, d_q_offsets_ptr, nq, q_nvalues, d_hits_ptr, cap_hits, min_shared=1, d_q_min_ptr=None, stream=None):
        """Resident CSR queries (raw device pointers; d_q_min: nq int32 or None; d_hits: cap_hits rows of 3 int32) -> the total number
        of hits; the first min(total, cap_hits) are written, in order.  Runs on `stream` (as for compare_sketches_device) and
        synchronises it.  Query rows are clamped to [0, q_nvalues] on the device."""
        if stream is None:
            stream = self._ctx.stream
        n = C.c_uint64()
        _chk(self._lib.rk_search_scaled_device(self._ctx._h, self._h, C.c_void_p(d_q_values_ptr), C.c_void_p(d_q_offsets_ptr), int(nq),
                                               C.c_uint64(int(q_nvalues)), int(min_shared), C.c_void_p(d_q_min_ptr), C.c_void_p(d_hits_ptr),
                                               C.c_uint64(int(cap_hits)), C.byref(n), C.c_void_p(stream)))
        return int(n.value)

    def multigather(self, q_values, q_offsets, q_abund=None, min_shared=1, max_rounds=None):
        """rk_multigather_scaled: Context.gather_scaled for every row of the CSR query batch against the indexed references, all
        queries at once -> (rows int32 [n, 4], row_offsets uint64 [nq + 1], wunique uint64 [n] or None): the rows (reference, unique,
        total, remaining) of query i are rows[row_offsets[i]:row_offsets[i + 1]], in pick order; with q_abund (uint32, one per value)
        wunique as gather_scaled_abund gives it."""
        q_values, q_offsets, q_abund, nq, max_rounds, ro = _multigather_args(q_values, q_offsets, q_abund, max_rounds)
        out, wu, n = _i32p(), _u64p(), C.c_uint64()
        _chk(self._lib.rk_multigather_scaled(self._ctx._h, self._h, _p(q_values, C.c_uint64), None if q_abund is None else _p(q_abund, C.c_uint32),
                                             _p(q_offsets, C.c_uint64), nq, int(min_shared), max_rounds, C.byref(out), C.byref(wu), _p(ro, C.c_uint64),
                                             C.byref(n)))
        rows, w = _multigather_rows(self._lib, out, wu, int(n.value), q_abund is not None)
        return rows, ro, w

    def multigather_device(self, d_q_values_ptr, d_q_offsets_ptr, nq, q_nvalues, d_out4_ptr, d_row_offsets_ptr, cap_rows, d_q_abund_ptr=None,
                           d_wunique_ptr=None, min_shared=1, max_rounds=None, stream=None):
        """Resident CSR queries (raw device pointers; d_q_abund: q_nvalues uint32 or None; d_out4: cap_rows rows of 4 int32; d_wunique:
        cap_rows uint64, with d_q_abund; d_row_offsets: nq + 1 uint64) -> the total number of rows; the first min(total, cap_rows) are
        written, in order, and all of d_row_offsets.  Runs on `stream` (as for search_device) and synchronises it.  Query rows are
        clamped to [0, q_nvalues] on the device."""
        if stream is None:
            stream = self._ctx.stream
        n = C.c_uint64()
        _chk(self._lib.rk_multigather_scaled_device(self._ctx._h, self._h, C.c_void_p(d_q_values_ptr), C.c_void_p(d_q_abund_ptr), C.c_void_p(d_q_offsets_ptr),
                                                    int(nq), C.c_uint64(int(q_nvalues)), int(min_shared), 0x7fffffff if max_rounds is None else int(max_rounds),
                                                    C.c_void_p(d_out4_ptr), C.c_void_p(d_wunique_ptr), C.c_uint64(int(cap_rows)), C.c_void_p(d_row_offsets_ptr),
                                                    C.byref(n), C.c_void_p(stream)))
        return int(n.value)

    def cluster(self, r_values, r_offsets, min_shared=1, measure=RK_CLUSTER_JACCARD, min_ppm=0, hit_cap=0):
        """rk_cluster_scaled: the collection the index was made from (the same CSR arrays) searched against the index and grouped
        into single-linkage clusters -> int32 [nref]: the smallest index of every sketch's cluster.  The hits stay on the device,
        never more than hit_cap of them at once (0: the library's default)."""
        r_values, r_offsets = _csr(r_values, r_offsets)
        labels = np.zeros(max(len(r_offsets) - 1, 1), dtype=np.int32)
        _chk(self._lib.rk_cluster_scaled(self._ctx._h, self._h, _p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), len(r_offsets) - 1, int(min_shared),
                                         int(measure), C.c_uint32(int(min_ppm)), C.c_uint64(int(hit_cap)), _p(labels, C.c_int32)))
        return labels[: len(r_offsets) - 1]

    def cluster_device(self, d_values_ptr, d_offsets_ptr, nref, nvalues, d_labels_ptr, min_shared=1, measure=RK_CLUSTER_JACCARD, min_ppm=0, hit_cap=0,
                       stream=None):
        """rk_cluster_scaled_device: the same on the resident CSR arrays of the collection (raw device pointers; d_labels: nref int32).
        Runs on `stream` (as for search_device) and synchronises it.  Rows are clamped to [0, nvalues] on the device."""
        if stream is None:
            stream = self._ctx.stream
        _chk(self._lib.rk_cluster_scaled_device(self._ctx._h, self._h, C.c_void_p(d_values_ptr), C.c_void_p(d_offsets_ptr), int(nref),
                                                C.c_uint64(int(nvalues)), int(min_shared), int(measure), C.c_uint32(int(min_ppm)),
                                                C.c_uint64(int(hit_cap)), C.c_void_p(d_labels_ptr), C.c_void_p(stream)))


class ScreenStats(C.Structure):
    """rk_screen_stats_t (rkmh_amd.h, "SCREEN")"""
    _fields_ = [("struct_size", C.c_uint32), ("nref", C.c_uint32), ("dir_shift", C.c_uint32), ("dir_buckets", C.c_uint32), ("nkeys", C.c_uint64),
                ("nseq", C.c_uint64), ("nbases", C.c_uint64), ("counted", C.c_uint64), ("injected", C.c_uint64)]


def screen_rows_host(r_values, r_offsets, c_values, c_counts, min_copies=1):
    """rk_screen_rows_host (host code, no GPU): the CSR reference rows against a counted set (values uint64 ascending, counts uint64)
    -> uint32 [nref, 4]: (shared, median, owned shared, owned median) per reference."""
    r_values, r_offsets = _csr(r_values, r_offsets)
    c_values = np.ascontiguousarray(c_values, dtype=np.uint64)
    c_counts = np.ascontiguousarray(c_counts, dtype=np.uint64)
    if c_values.ndim != 1 or c_counts.shape != c_values.shape:
        raise ValueError("values and counts must be one-dimensional and of one length")
    if not 0 <= int(min_copies) < 1 << 64:
        raise ValueError("min_copies outside the range of uint64")
    nref = len(r_offsets) - 1
    out = np.zeros((max(nref, 1), 4), dtype=np.uint32)
    _chk(load_library().rk_screen_rows_host(_p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), nref, _p(c_values, C.c_uint64), _p(c_counts, C.c_uint64),
                                            len(c_values), C.c_uint64(int(min_copies)), _p(out, C.c_uint32)))
    return out[:max(nref, 0)]


def screen_identity(shared, length, k):
    """rk_screen_identity (host code): (shared / length)^(1 / k); 0 when nothing is shared, 1 when everything is."""
    d = C.c_double()
    _chk(load_library().rk_screen_identity(C.c_uint64(int(shared)), C.c_uint64(int(length)), int(k), C.byref(d)))
    return float(d.value)


class Screen:
    """rk_screen: reference sketches (CSR rows, ascending, repeats allowed) resident as the keys of an inverted index, and one 64-bit
    counter per key that the window hashes of the reads fed are counted into (Context.screen; rkmh_amd.h "SCREEN")."""

    def __init__(self, ctx, ks, r_values, r_offsets):
        self._ctx, self._lib = ctx, ctx._lib
        ks = _ks(ks)
        r_values, r_offsets = _csr(r_values, r_offsets)
        self.nref = len(r_offsets) - 1
        self._h = C.c_void_p()
        _chk(self._lib.rk_screen_create(ctx._h, _p(ks, C.c_int), len(ks), _p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), self.nref, C.byref(self._h)))

    def add(self, bases, offsets):
        """rk_screen_add_batch: host bases (uint8) and uint64 offsets[n + 1]; refuses offsets that reach past the bases."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError("offsets must hold n + 1 entries")
        bases = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, dtype=np.uint8)
        if int(offsets.max()) > len(bases):
            raise ValueError("offsets reach past the %d bases" % len(bases))
        _chk(self._lib.rk_screen_add_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), len(offsets) - 1))

    def add_device(self, d_bases_ptr, d_offsets_ptr, nseq, stream=None):
        """rk_screen_add_batch_device: resident bases and uint32 offsets[nseq + 1]; asynchronous on the stream."""
        _chk(self._lib.rk_screen_add_batch_device(self._h, C.c_void_p(d_bases_ptr), C.c_void_p(d_offsets_ptr), int(nseq), C.c_void_p(stream or 0)))

    def add_counts(self, values, counts):
        """rk_screen_add_counts: multiplicities (uint32) for ascending distinct values; values that are no key are ignored."""
        values, counts = _value_counts(values, counts)
        _chk(self._lib.rk_screen_add_counts(self._h, _p(values, C.c_uint64), _p(counts, C.c_uint32), len(values)))

    def rows(self, min_copies=1):
        """rk_screen_rows -> uint32 [nref, 4]: (shared, median, owned shared, owned median) per reference; the screen stays usable."""
        if not 0 <= int(min_copies) < 1 << 64:
            raise ValueError("min_copies outside the range of uint64")
        out = np.zeros((max(self.nref, 1), 4), dtype=np.uint32)
        _chk(self._lib.rk_screen_rows(self._h, C.c_uint64(int(min_copies)), _p(out, C.c_uint32)))
        return out[:self.nref]

    def rows_device(self, d_out4_ptr, min_copies=1, stream=None):
        """rk_screen_rows_device: the same into nref * 4 uint32 on the device; runs on the stream and does not synchronise it."""
        _chk(self._lib.rk_screen_rows_device(self._h, C.c_uint64(int(min_copies)), C.c_void_p(d_out4_ptr), C.c_void_p(stream or 0)))

    def counts(self):
        """rk_screen_counts -> (keys uint64 ascending, counts uint64: raw, not clamped)"""
        ok, oc, n = _u64p(), _u64p(), C.c_uint64()
        _chk(self._lib.rk_screen_counts(self._h, C.byref(ok), C.byref(oc), C.byref(n)))
        m = int(n.value)
        k = np.ctypeslib.as_array(ok, shape=(max(m, 1),))[:m].copy()
        c = np.ctypeslib.as_array(oc, shape=(max(m, 1),))[:m].copy()
        self._lib.rk_free(ok)
        self._lib.rk_free(oc)
        return k, c

    def stats(self):
        """-> dict(nref, nkeys, dir_shift, dir_buckets, nseq, nbases, counted, injected)"""
        s = ScreenStats()
        s.struct_size = C.sizeof(ScreenStats)
        _chk(self._lib.rk_screen_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("nref", "nkeys", "dir_shift", "dir_buckets", "nseq", "nbases", "counted", "injected")}

    def reset(self):
        _chk(self._lib.rk_screen_reset(self._h))

    def close(self):
        if self._h:
            self._lib.rk_screen_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _abund(abund, values):
    """the abundances that lie parallel to `values`: uint32, one per value"""
    abund = np.ascontiguousarray(abund, dtype=np.uint32)
    if abund.ndim != 1 or len(abund) != len(values):
        raise ValueError("%d abundances for %d values" % (abund.size, len(values)))
    return abund


def merge_scaled_abund(values, abunds, offsets, max_hash=(1 << 64) - 1):
    """rk_merge_scaled_abund (host code, no GPU): merge_scaled's values plus, per value, the sum of its abundances over the sketches,
    saturating at 2^32 - 1 -> (values uint64, abunds uint32)."""
    values, offsets = _csr(values, offsets)
    abunds = _abund(abunds, values)
    out, oa, n = _u64p(), _u32p(), C.c_uint64()
    lib = load_library()
    _chk(lib.rk_merge_scaled_abund(_p(values, C.c_uint64), _p(abunds, C.c_uint32), _p(offsets, C.c_uint64), len(offsets) - 1, C.c_uint64(int(max_hash)),
                                   C.byref(out), C.byref(oa), C.byref(n)))
    m = int(n.value)
    r = np.ctypeslib.as_array(out, shape=(max(m, 1),))[:m].copy()
    a = np.ctypeslib.as_array(oa, shape=(max(m, 1),))[:m].copy()
    lib.rk_free(out)
    lib.rk_free(oa)
    return r, a


def gather_scaled_abund_host(q, q_abund, r_values, r_offsets, min_shared=1, max_rounds=None, threads=1):
    """rk_gather_scaled_abund_host (host code, no GPU): the rows of gather_scaled_host and, per row, wunique = the summed abundances
    of the query values that pick removes -> (int32 [n, 4], uint64 [n])."""
    q, r_values, r_offsets, nref, max_rounds, out = _gather_args(q, r_values, r_offsets, max_rounds)
    q_abund = _abund(q_abund, q)
    wu = np.zeros(len(out), dtype=np.uint64)
    n = C.c_int(0)
    _chk(load_library().rk_gather_scaled_abund_host(_p(q, C.c_uint64), _p(q_abund, C.c_uint32), len(q), _p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64),
                                                    nref, int(min_shared), max_rounds, int(threads), _p(out, C.c_int32), _p(wu, C.c_uint64), C.byref(n)))
    return out[: n.value].copy(), wu[: n.value].copy()


def _abund_sides(a_values, a_abund, a_offsets, b_values, b_abund, b_offsets):
    """both sides of a weighted comparison, checked (b None: a itself, the same arrays) -> (av, aw, ao, bv, bw, bo, out uint64 [na, nb, 4])"""
    a_values, a_offsets = _csr(a_values, a_offsets)
    a_abund = _abund(a_abund, a_values)
    if b_values is None:
        if b_abund is not None or b_offsets is not None:
            raise ValueError("b_abund and b_offsets go with b_values")
        b_values, b_abund, b_offsets = a_values, a_abund, a_offsets
    else:
        b_values, b_offsets = _csr(b_values, b_offsets)
        b_abund = _abund(b_abund, b_values)
    out = np.zeros((max(len(a_offsets) - 1, 0), max(len(b_offsets) - 1, 0), 4), dtype=np.uint64)
    return a_values, a_abund, a_offsets, b_values, b_abund, b_offsets, out


def _abund_rows(abund, offsets):
    abund = np.ascontiguousarray(abund, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if abund.ndim != 1 or len(offsets) < 1 or int(offsets.max()) > len(abund):
        raise ValueError("offsets run past the %d abundances" % abund.size)
    return abund, offsets, np.zeros((len(offsets) - 1, 2), dtype=np.uint64)


def compare_scaled_abund_host(a_values, a_abund, a_offsets, b_values=None, b_abund=None, b_offsets=None, threads=1):
    """rk_compare_scaled_abund_host (host code, no GPU): what Context.compare_scaled_abund gives, from plain loops on `threads` host threads."""
    av, aw, ao, bv, bw, bo, out = _abund_sides(a_values, a_abund, a_offsets, b_values, b_abund, b_offsets)
    _chk(load_library().rk_compare_scaled_abund_host(_p(av, C.c_uint64), _p(aw, C.c_uint32), _p(ao, C.c_uint64), len(ao) - 1, _p(bv, C.c_uint64),
                                                     _p(bw, C.c_uint32), _p(bo, C.c_uint64), len(bo) - 1, int(threads), _p(out, C.c_uint64)))
    return out


def abund_row_sums_host(abund, offsets):
    """rk_abund_row_sums_host (host code, no GPU): uint64 [n, 2], per CSR row of abundances (sum, sum of squares saturating at 2^64 - 1)."""
    abund, offsets, out = _abund_rows(abund, offsets)
    _chk(load_library().rk_abund_row_sums_host(_p(abund, C.c_uint32), _p(offsets, C.c_uint64), len(offsets) - 1, _p(out, C.c_uint64)))
    return out


def angular_similarity(dot, sumsq_a, sumsq_b):
    """rk_angular_similarity (host code, no GPU): (cosine, angular) = (dot / sqrt(sumsq_a * sumsq_b) clamped to 1, 1 - 2 acos(cosine) / pi);
    both 0 when a sumsq is 0."""
    c, a = C.c_double(), C.c_double()
    _chk(load_library().rk_angular_similarity(C.c_uint64(int(dot)), C.c_uint64(int(sumsq_a)), C.c_uint64(int(sumsq_b)), C.byref(c), C.byref(a)))
    return c.value, a.value


def _value_counts(values, counts):
    values = np.ascontiguousarray(values, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if values.ndim != 1 or counts.shape != values.shape:
        raise ValueError("values and counts must be one-dimensional and of one length")
    return values, counts


def bottom_cut(values, counts, sketch_size, min_copies=1, distinct=False, ctx=None):
    """rk_bottom_cut: where the bottom sketch_size of the sorted distinct set (values uint64 ascending, counts uint32) ends, found on
    the GPU -> (cut_len, threshold); cut_len = 0: no cut.  ctx: the Context to run on; None makes one on device 0 for the call."""
    values, counts = _value_counts(values, counts)
    own = ctx is None
    if own:
        ctx = Context(0)
    try:
        n, t = C.c_uint64(), C.c_uint64()
        _chk(ctx._lib.rk_bottom_cut(ctx._h, _p(values, C.c_uint64), _p(counts, C.c_uint32), len(values), int(sketch_size), C.c_uint64(int(min_copies)),
                                    1 if distinct else 0, C.byref(n), C.byref(t)))
        return int(n.value), int(t.value)
    finally:
        if own:
            ctx.close()


def bottom_emit(values, counts, sketch_size, min_copies=1, distinct=False):
    """rk_bottom_emit (host code, no GPU): the bottom-s row of a sorted distinct (values, counts) set -> (uint64 [sketch_size], length)."""
    values, counts = _value_counts(values, counts)
    row = np.zeros(max(int(sketch_size), 1), dtype=np.uint64)
    m = C.c_int32()
    _chk(load_library().rk_bottom_emit(_p(values, C.c_uint64), _p(counts, C.c_uint32), len(values), int(sketch_size), C.c_uint64(int(min_copies)),
                                       1 if distinct else 0, _p(row, C.c_uint64), C.byref(m)))
    return row[:max(int(sketch_size), 0)], int(m.value)


class SampleStats(C.Structure):
    """rk_sample_stats_t (rkmh_amd.h, "SAMPLE SKETCHES")"""
    _fields_ = [("struct_size", C.c_uint32), ("folds", C.c_uint32), ("retries", C.c_uint32), ("reserved", C.c_uint32), ("nseq", C.c_uint64),
                ("nbases", C.c_uint64), ("kept", C.c_uint64), ("distinct", C.c_uint64)]


class Sample:
    """rk_sample: one scaled sketch, with or without abundances, accumulated on the device from the reads fed to it (Context.sample);
    or, with sketch_size, a bottom sample (Context.sample_bottom; rkmh_amd.h "BOTTOM SAMPLES"): one bottom-s sketch of the values seen at
    least min_copies times, which always keeps counts."""

    def __init__(self, ctx, ks, max_hash, abund=False, pending_cap=0, sketch_size=None, min_copies=1):
        self._ctx, self._lib = ctx, ctx._lib
        self.abund = bool(abund) or sketch_size is not None
        self.sketch_size = None if sketch_size is None else int(sketch_size)
        ks = _ks(ks)
        self._h = C.c_void_p()
        if sketch_size is not None:
            if not 0 <= int(min_copies) < 1 << 64:
                raise ValueError("min_copies outside the range of uint64")
            _chk(self._lib.rk_sample_create_bottom(ctx._h, _p(ks, C.c_int), len(ks), max(min(int(sketch_size), 2 ** 31 - 1), -2 ** 31),
                                                   C.c_uint64(int(min_copies)), C.c_uint64(int(pending_cap)), C.byref(self._h)))
            return
        _chk(self._lib.rk_sample_create(ctx._h, _p(ks, C.c_int), len(ks), C.c_uint64(int(max_hash)), 1 if abund else 0, C.c_uint64(int(pending_cap)),
                                        C.byref(self._h)))

    def add(self, bases, offsets):
        """rk_sample_add_batch: host bases (uint8) and uint64 offsets[n + 1]; refuses offsets that reach past the bases."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError("offsets must hold n + 1 entries")
        bases = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, dtype=np.uint8)
        if int(offsets.max()) > len(bases):
            raise ValueError("offsets reach past the %d bases" % len(bases))
        _chk(self._lib.rk_sample_add_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), len(offsets) - 1))

    def add_device(self, d_bases_ptr, d_offsets_ptr, nseq, stream=None):
        """rk_sample_add_batch_device: resident bases and uint32 offsets[nseq + 1]; synchronises the stream."""
        _chk(self._lib.rk_sample_add_batch_device(self._h, C.c_void_p(d_bases_ptr), C.c_void_p(d_offsets_ptr), int(nseq), C.c_void_p(stream or 0)))

    def add_sketch(self, values, abund=None):
        """rk_sample_add_sketch: an abundance sketch (or, for a sample without abundances, a plain one) united into the sample."""
        values = np.ascontiguousarray(values, dtype=np.uint64)
        if values.ndim != 1:
            raise ValueError("values must be one-dimensional")
        if abund is not None:
            abund = _abund(abund, values)
        _chk(self._lib.rk_sample_add_sketch(self._h, _p(values, C.c_uint64), None if abund is None else _p(abund, C.c_uint32), len(values)))

    def finish(self):
        """rk_sample_finish -> (values uint64, abund uint32 or None); the sample stays usable."""
        out, oa, n = _u64p(), _u32p(), C.c_uint64()
        _chk(self._lib.rk_sample_finish(self._h, C.byref(out), C.byref(oa), C.byref(n)))
        m = int(n.value)
        r = np.ctypeslib.as_array(out, shape=(max(m, 1),))[:m].copy()
        self._lib.rk_free(out)
        a = None
        if self.abund:
            a = np.ctypeslib.as_array(oa, shape=(max(m, 1),))[:m].copy()
            self._lib.rk_free(oa)
        return r, a

    def finish_bottom(self):
        """rk_sample_finish_bottom -> (row uint64 [sketch_size], zero padded, length); the sample stays usable."""
        if self.sketch_size is None:
            raise RkmhError("a scaled sample has no bottom-s row")
        row = np.zeros(self.sketch_size, dtype=np.uint64)
        m = C.c_int32()
        _chk(self._lib.rk_sample_finish_bottom(self._h, _p(row, C.c_uint64), C.byref(m)))
        return row, int(m.value)

    def bottom_state(self):
        """rk_sample_bottom_state -> dict(threshold, candidates, qualifying_weight, cuts)"""
        t, n, w, c = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        _chk(self._lib.rk_sample_bottom_state(self._h, C.byref(t), C.byref(n), C.byref(w), C.byref(c)))
        return dict(threshold=int(t.value), candidates=int(n.value), qualifying_weight=int(w.value), cuts=int(c.value))

    def device(self):
        """rk_sample_device -> (device pointer of the values, of the abundances or None, n): valid until the next add, reset or close."""
        dv, da, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _chk(self._lib.rk_sample_device(self._h, C.byref(dv), C.byref(da), C.byref(n)))
        return dv.value, da.value, int(n.value)

    def stats(self):
        """-> dict(folds, retries, nseq, nbases, kept, distinct)"""
        s = SampleStats()
        s.struct_size = C.sizeof(SampleStats)
        _chk(self._lib.rk_sample_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k in ("folds", "retries", "nseq", "nbases", "kept", "distinct")}

    def reset(self):
        _chk(self._lib.rk_sample_reset(self._h))

    def close(self):
        if self._h:
            self._lib.rk_sample_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One GPU. Methods are named after the reference's functions they replace."""

    def __init__(self, device=0, policy_spec=None, **policy):
        """policy_spec: the text form (`--hash-policy` of the command lines: presets default / mash / sourmash, key=value; rk_policy_parse),
        applied to the defaults first; keyword arguments then set single fields of the struct."""
        self._lib = load_library()
        p = parse_policy(policy_spec)
        for k, v in policy.items():
            setattr(p, k, v)
        self.policy = p
        self._h = C.c_void_p()
        _chk(self._lib.rk_ctx_create(device, C.byref(p), C.byref(self._h)))
        self.sketch_size = None
        self.ks = None

    def close(self):
        if self._h:
            self._lib.rk_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _chk(self._lib.rk_ctx_synchronize(self._h))

    # ---- inner boundary (mkmh mirrors) -------------------------------------------------------
    def to_upper(self, s: bytes) -> bytes:
        b = C.create_string_buffer(s, len(s))
        _chk(self._lib.rk_to_upper(self._h, b, len(s)))
        return b.raw

    def calc_hashes(self, seq: bytes, ks, counter=None) -> np.ndarray:
        ks = _ks(ks)
        out = _u64p()
        n = C.c_int()
        if counter is None:
            _chk(self._lib.rk_calc_hashes(self._h, seq, len(seq), _p(ks, C.c_int), len(ks), C.byref(out), C.byref(n)))
        else:
            _chk(self._lib.rk_calc_hashes_counted(self._h, seq, len(seq), _p(ks, C.c_int), len(ks), C.byref(out),
                                                  C.byref(n), counter._h))
        r = np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[: n.value].copy()
        self._lib.rk_free(out)
        return r

    def calc_hash(self, kmer: bytes) -> int:
        v = C.c_uint64()
        _chk(self._lib.rk_calc_hash(self._h, kmer, len(kmer), C.byref(v)))
        return int(v.value)

    def minhashes(self, h: np.ndarray, sketch_size: int, counter=None, min_count=0, max_count=0):
        """Returns (mins, sorted_input) -- the reference sorts its input in place."""
        h = np.ascontiguousarray(h, dtype=np.uint64).copy()
        out = _u64p()
        m = C.c_int()
        if counter is None:
            _chk(self._lib.rk_minhashes(self._h, _p(h, C.c_uint64), len(h), sketch_size, C.byref(out), C.byref(m)))
        else:
            _chk(self._lib.rk_minhashes_frequency_filter(self._h, _p(h, C.c_uint64), len(h), sketch_size, C.byref(out),
                                                         C.byref(m), counter._h, min_count, max_count))
        r = np.ctypeslib.as_array(out, shape=(max(sketch_size, 1),))[: m.value].copy()
        self._lib.rk_free(out)
        return r, h

    def mask_by_frequency(self, h: np.ndarray, counter, min_occ: int) -> np.ndarray:
        h = np.ascontiguousarray(h, dtype=np.uint64).copy()
        _chk(self._lib.rk_mask_by_frequency(self._h, _p(h, C.c_uint64), len(h), counter._h, min_occ))
        return h

    def hash_intersection_size(self, a, b) -> int:
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        out = C.c_int()
        _chk(self._lib.rk_hash_intersection_size(self._h, _p(a, C.c_uint64), len(a), _p(b, C.c_uint64), len(b), C.byref(out)))
        return out.value

    def hash_intersection(self, a, a_start, a_len, b, b_start, b_len, sketch_size):
        """mkmh's 7-argument hash_intersection (equiv.hpp:308,340,364): the matches themselves (<= sketch_size)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        if a_start < 0 or b_start < 0 or a_start + a_len > len(a) or b_start + b_len > len(b):
            raise ValueError("range outside the array")
        out, n = _u64p(), C.c_int()
        _chk(self._lib.rk_hash_intersection(self._h, _p(a, C.c_uint64), a_start, a_len, _p(b, C.c_uint64), b_start, b_len,
                                            sketch_size, C.byref(out), C.byref(n)))
        r = np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[: n.value].copy()
        self._lib.rk_free(out)
        return r

    # ---- sketch comparison ---------------------------------------------------------------------
    def compare_sketches(self, a, alens, b=None, blens=None, sketch_size=None):
        """rk_compare_sketches: every row of `a` (uint64 [na, sketch_size], lengths alens) against every row of `b` (None: of `a`
        itself) -> int32 [na, nb, 4] = (shared, shared_distinct, common, denom) per pair."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        alens = np.ascontiguousarray(alens, dtype=np.int32)
        if sketch_size is None:
            sketch_size = a.shape[1]
        if b is None:
            b, blens = a, alens
        else:
            b = np.ascontiguousarray(b, dtype=np.uint64)
            blens = np.ascontiguousarray(blens, dtype=np.int32)
        na, nb = len(alens), len(blens)
        if a.size != na * sketch_size or b.size != nb * sketch_size:
            raise ValueError("sketch arrays must hold len(lens) rows of sketch_size values")
        out = np.zeros((na, nb, 4), dtype=np.int32)
        _chk(self._lib.rk_compare_sketches(self._h, _p(a, C.c_uint64), _p(alens, C.c_int32), na, _p(b, C.c_uint64), _p(blens, C.c_int32), nb,
                                           sketch_size, _p(out, C.c_int32)))
        return out

    def compare_sketches_device(self, d_a_ptr, d_alens_ptr, na, d_b_ptr, d_blens_ptr, nb, sketch_size, d_out_ptr, stream=None):
        """Resident arrays (raw device pointers; d_out: na * nb * 4 int32); asynchronous.  stream: a hipStream_t handle (e.g.
        torch.cuda.current_stream().cuda_stream; 0 = null stream); None = the context's own stream, as for classify_device."""
        if stream is None:
            stream = self.stream
        _chk(self._lib.rk_compare_sketches_device(self._h, C.c_void_p(d_a_ptr), C.c_void_p(d_alens_ptr), na, C.c_void_p(d_b_ptr),
                                                  C.c_void_p(d_blens_ptr), nb, sketch_size, C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    # ---- scaled sketches -----------------------------------------------------------------------
    def sketch_scaled_batch(self, bases, offsets, ks, max_hash):
        """rk_sketch_scaled_batch: the distinct window hashes 0 < h <= max_hash of every sequence, ascending -> (values uint64,
        offsets uint64 [n + 1]): sketch i is values[offsets[i]:offsets[i + 1]]."""
        ks = _ks(ks)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        so = np.zeros(n + 1, dtype=np.uint64)
        out = _u64p()
        _chk(self._lib.rk_sketch_scaled_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), n, _p(ks, C.c_int), len(ks),
                                              C.c_uint64(int(max_hash)), C.byref(out), _p(so, C.c_uint64)))
        tot = int(so[-1])
        r = np.ctypeslib.as_array(out, shape=(max(tot, 1),))[:tot].copy()
        self._lib.rk_free(out)
        return r, so

    def sketch_scaled_abund_batch(self, bases, offsets, ks, max_hash):
        """rk_sketch_scaled_abund_batch: sketch_scaled_batch's (values, offsets) and abunds uint32, parallel to the values: the number
        of windows of the sequence that hash to each -> (values, abunds, offsets)."""
        ks = _ks(ks)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        so = np.zeros(n + 1, dtype=np.uint64)
        out, oa = _u64p(), _u32p()
        _chk(self._lib.rk_sketch_scaled_abund_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), n, _p(ks, C.c_int), len(ks),
                                                    C.c_uint64(int(max_hash)), C.byref(out), C.byref(oa), _p(so, C.c_uint64)))
        tot = int(so[-1])
        r = np.ctypeslib.as_array(out, shape=(max(tot, 1),))[:tot].copy()
        a = np.ctypeslib.as_array(oa, shape=(max(tot, 1),))[:tot].copy()
        self._lib.rk_free(out)
        self._lib.rk_free(oa)
        return r, a, so

    def sample(self, ks, max_hash, abund=False, pending_cap=0):
        """rk_sample_create: an empty Sample at (ks, this context's policy, max_hash); pending_cap 0 = the library's default."""
        return Sample(self, ks, max_hash, abund=abund, pending_cap=pending_cap)

    def screen(self, ks, r_values, r_offsets):
        """rk_screen_create -> Screen: the CSR reference rows resident, every count 0."""
        return Screen(self, ks, r_values, r_offsets)

    def sample_bottom(self, ks, sketch_size, min_copies=1, pending_cap=0):
        """rk_sample_create_bottom: an empty bottom sample at (ks, this context's policy, sketch_size, min_copies)."""
        return Sample(self, ks, 0, pending_cap=pending_cap, sketch_size=sketch_size, min_copies=min_copies)

    def bottom_cut(self, values, counts, sketch_size, min_copies=1, distinct=False):
        """rk_bottom_cut on this context: see the module's bottom_cut."""
        return bottom_cut(values, counts, sketch_size, min_copies, distinct, ctx=self)

    def compare_scaled(self, a_values, a_offsets, b_values=None, b_offsets=None, lanes=0):
        """rk_compare_scaled: every CSR sketch of `a` against every one of `b` (None: of `a` itself) -> int32 [na, nb], the number
        of shared values.  lanes: 0 (chosen from the lengths), 1, 8 or 64 lanes of the kernel per pair; the answer is the same."""
        a_values, a_offsets = _csr(a_values, a_offsets)
        if b_values is None:
            b_values, b_offsets = a_values, a_offsets
        else:
            b_values, b_offsets = _csr(b_values, b_offsets)
        na, nb = len(a_offsets) - 1, len(b_offsets) - 1
        out = np.zeros((max(na, 0), max(nb, 0)), dtype=np.int32)
        _chk(self._lib.rk_compare_scaled(self._h, _p(a_values, C.c_uint64), _p(a_offsets, C.c_uint64), na, _p(b_values, C.c_uint64),
                                         _p(b_offsets, C.c_uint64), nb, int(lanes), _p(out, C.c_int32)))
        return out

    def compare_scaled_device(self, d_a_values_ptr, d_a_offsets_ptr, na, a_nvalues, d_b_values_ptr, d_b_offsets_ptr, nb, b_nvalues,
                              d_shared_ptr, lanes=0, stream=None):
        """Resident CSR arrays (raw device pointers; d_shared: na * nb int32); asynchronous.  Rows are clamped to [0, nvalues] on the
        device.  stream as for compare_sketches_device."""
        if stream is None:
            stream = self.stream
        _chk(self._lib.rk_compare_scaled_device(self._h, C.c_void_p(d_a_values_ptr), C.c_void_p(d_a_offsets_ptr), na, C.c_uint64(int(a_nvalues)),
                                                C.c_void_p(d_b_values_ptr), C.c_void_p(d_b_offsets_ptr), nb, C.c_uint64(int(b_nvalues)),
                                                int(lanes), C.c_void_p(d_shared_ptr), C.c_void_p(stream)))

    # ---- weighted comparison ---------------------------------------------------------------------
    def compare_scaled_abund(self, a_values, a_abund, a_offsets, b_values=None, b_abund=None, b_offsets=None, lanes=0):
        """rk_compare_scaled_abund: every CSR abundance sketch of `a` against every one of `b` (None: of `a` itself) -> uint64
        [na, nb, 4]: (shared, dot = sum of wA * wB over the shared values, saturating at 2^64 - 1, wa_in, wb_in = the abundances of the
        shared values summed per side).  lanes as for compare_scaled; the answer is the same."""
        av, aw, ao, bv, bw, bo, out = _abund_sides(a_values, a_abund, a_offsets, b_values, b_abund, b_offsets)
        _chk(self._lib.rk_compare_scaled_abund(self._h, _p(av, C.c_uint64), _p(aw, C.c_uint32), _p(ao, C.c_uint64), len(ao) - 1, _p(bv, C.c_uint64),
                                               _p(bw, C.c_uint32), _p(bo, C.c_uint64), len(bo) - 1, int(lanes), _p(out, C.c_uint64)))
        return out

    def compare_scaled_abund_device(self, d_a_values_ptr, d_a_abund_ptr, d_a_offsets_ptr, na, a_nvalues, d_b_values_ptr, d_b_abund_ptr, d_b_offsets_ptr,
                                    nb, b_nvalues, d_out4_ptr, lanes=0, stream=None):
        """Resident CSR arrays and their abundances (raw device pointers; d_out4: na * nb * 4 uint64); asynchronous.  Rows are clamped to
        [0, nvalues] on the device; an abundance of 0 adds nothing.  stream as for compare_sketches_device."""
        if stream is None:
            stream = self.stream
        _chk(self._lib.rk_compare_scaled_abund_device(self._h, C.c_void_p(d_a_values_ptr), C.c_void_p(d_a_abund_ptr), C.c_void_p(d_a_offsets_ptr), na,
                                                      C.c_uint64(int(a_nvalues)), C.c_void_p(d_b_values_ptr), C.c_void_p(d_b_abund_ptr),
                                                      C.c_void_p(d_b_offsets_ptr), nb, C.c_uint64(int(b_nvalues)), int(lanes), C.c_void_p(d_out4_ptr),
                                                      C.c_void_p(stream)))

    def abund_row_sums(self, abund, offsets):
        """rk_abund_row_sums: uint64 [n, 2], per CSR row of abundances (sum, sum of squares saturating at 2^64 - 1)."""
        abund, offsets, out = _abund_rows(abund, offsets)
        _chk(self._lib.rk_abund_row_sums(self._h, _p(abund, C.c_uint32), _p(offsets, C.c_uint64), len(offsets) - 1, _p(out, C.c_uint64)))
        return out

    def abund_row_sums_device(self, d_abund_ptr, d_offsets_ptr, n, nvalues, d_out2_ptr, stream=None):
        """Resident arrays (raw device pointers; d_out2: n * 2 uint64); asynchronous; rows are clamped to [0, nvalues] on the device."""
        if stream is None:
            stream = self.stream
        _chk(self._lib.rk_abund_row_sums_device(self._h, C.c_void_p(d_abund_ptr), C.c_void_p(d_offsets_ptr), n, C.c_uint64(int(nvalues)),
                                                C.c_void_p(d_out2_ptr), C.c_void_p(stream)))

    # ---- search ----------------------------------------------------------------------------------
    def scaled_index(self, r_values, r_offsets):
        """rk_scaled_index_create: the inverted index of the CSR reference sketches, built on the device and resident until its
        close() -> ScaledIndex (stats, search, search_device)."""
        r_values, r_offsets = _csr(r_values, r_offsets)
        h = C.c_void_p()
        _chk(self._lib.rk_scaled_index_create(self._h, _p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), len(r_offsets) - 1, C.byref(h)))
        return ScaledIndex(self, h)

    def scaled_index_device(self, d_values_ptr, d_offsets_ptr, nref, nvalues, stream=None):
        """rk_scaled_index_create_device: the index of resident CSR reference sketches (raw device pointers, only read); rows are
        clamped to [0, nvalues] on the device.  Runs on `stream` and synchronises it."""
        if stream is None:
            stream = self.stream
        h = C.c_void_p()
        _chk(self._lib.rk_scaled_index_create_device(self._h, C.c_void_p(d_values_ptr), C.c_void_p(d_offsets_ptr), int(nref), C.c_uint64(int(nvalues)),
                                                     C.c_void_p(stream), C.byref(h)))
        return ScaledIndex(self, h)

    # ---- cluster ---------------------------------------------------------------------------------
    def cluster_hits(self, hits, lens, measure=RK_CLUSTER_JACCARD, min_ppm=0):
        """rk_cluster_hits: cluster_hits_host's answer from the device: the hits and lengths are uploaded, hooked and compressed to
        the fixpoint, the labels downloaded -> int32 [n]."""
        hits, lens, labels = _cluster_args(hits, lens)
        _chk(self._lib.rk_cluster_hits(self._h, _p(hits, C.c_int32), C.c_uint64(len(hits)), _p(lens, C.c_uint64), len(lens), int(measure),
                                       C.c_uint32(int(min_ppm)), _p(labels, C.c_int32)))
        return labels

    def cluster_hits_device(self, d_hits_ptr, nhits, d_offsets_ptr, n, nvalues, d_labels_ptr, measure=RK_CLUSTER_JACCARD, min_ppm=0, stream=None):
        """rk_cluster_hits_device: resident hits (raw device pointers; nhits rows of 3 int32), the collection's CSR offsets (n + 1
        uint64; rows clamped to [0, nvalues]) -> the number of hook launches; d_labels takes n int32.  Runs on `stream` (as for
        compare_sketches_device) and synchronises it."""
        if stream is None:
            stream = self.stream
        rounds = C.c_uint32()
        _chk(self._lib.rk_cluster_hits_device(self._h, C.c_void_p(d_hits_ptr), C.c_uint64(int(nhits)), C.c_void_p(d_offsets_ptr), int(n),
                                              C.c_uint64(int(nvalues)), int(measure), C.c_uint32(int(min_ppm)), C.c_void_p(d_labels_ptr),
                                              C.byref(rounds), C.c_void_p(stream)))
        return int(rounds.value)

    # ---- gather ----------------------------------------------------------------------------------
    def gather_scaled(self, q, r_values, r_offsets, min_shared=1, max_rounds=None):
        """rk_gather_scaled: the greedy decomposition of the scaled sketch q (ascending, distinct, non-zero) into the CSR reference
        sketches -> int32 [n, 4], one row per pick: (reference, unique = values of what is left of q that it holds, total = |q & ref|,
        remaining = values of q left after it).  Stops when the best reference holds fewer than min_shared of what is left, or after
        max_rounds rows (None: the number of references)."""
        q, r_values, r_offsets, nref, max_rounds, out = _gather_args(q, r_values, r_offsets, max_rounds)
        n = C.c_int(0)
        _chk(self._lib.rk_gather_scaled(self._h, _p(q, C.c_uint64), len(q), _p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64), nref,
                                        int(min_shared), max_rounds, _p(out, C.c_int32), C.byref(n)))
        return out[: n.value].copy()

    def gather_scaled_device(self, d_q_ptr, nq, d_r_values_ptr, d_r_offsets_ptr, nref, r_nvalues, d_out4_ptr, min_shared=1, max_rounds=None,
                             stream=None):
        """Resident arrays (raw device pointers; d_out4: max_rounds rows of 4 int32, None: nref rows) -> the number of rows written.
        Runs on `stream` (as for compare_sketches_device) and synchronises it.  Rows are clamped to [0, r_nvalues] on the device."""
        if stream is None:
            stream = self.stream
        n = C.c_int(0)
        _chk(self._lib.rk_gather_scaled_device(self._h, C.c_void_p(d_q_ptr), C.c_uint64(int(nq)), C.c_void_p(d_r_values_ptr), C.c_void_p(d_r_offsets_ptr),
                                               int(nref), C.c_uint64(int(r_nvalues)), int(min_shared), int(nref if max_rounds is None else max_rounds),
                                               C.c_void_p(d_out4_ptr), C.byref(n), C.c_void_p(stream)))
        return n.value

    def gather_scaled_abund(self, q, q_abund, r_values, r_offsets, min_shared=1, max_rounds=None):
        """rk_gather_scaled_abund: gather_scaled's rows and, per row, wunique = the summed abundances (q_abund: uint32, one per value of
        q, none 0) of the query values that pick removes -> (int32 [n, 4], uint64 [n])."""
        q, r_values, r_offsets, nref, max_rounds, out = _gather_args(q, r_values, r_offsets, max_rounds)
        q_abund = _abund(q_abund, q)
        wu = np.zeros(len(out), dtype=np.uint64)
        n = C.c_int(0)
        _chk(self._lib.rk_gather_scaled_abund(self._h, _p(q, C.c_uint64), _p(q_abund, C.c_uint32), len(q), _p(r_values, C.c_uint64), _p(r_offsets, C.c_uint64),
                                              nref, int(min_shared), max_rounds, _p(out, C.c_int32), _p(wu, C.c_uint64), C.byref(n)))
        return out[: n.value].copy(), wu[: n.value].copy()

    def gather_scaled_abund_device(self, d_q_ptr, d_q_abund_ptr, nq, d_r_values_ptr, d_r_offsets_ptr, nref, r_nvalues, d_out4_ptr, d_wunique_ptr,
                                   min_shared=1, max_rounds=None, stream=None):
        """gather_scaled_device with the query's abundances (d_q_abund: nq uint32) and d_wunique (max_rounds uint64, None: nref) -> the
        number of rows written.  An abundance of 0 adds nothing."""
        if stream is None:
            stream = self.stream
        n = C.c_int(0)
        _chk(self._lib.rk_gather_scaled_abund_device(self._h, C.c_void_p(d_q_ptr), C.c_void_p(d_q_abund_ptr), C.c_uint64(int(nq)), C.c_void_p(d_r_values_ptr),
                                                     C.c_void_p(d_r_offsets_ptr), int(nref), C.c_uint64(int(r_nvalues)), int(min_shared),
                                                     int(nref if max_rounds is None else max_rounds), C.c_void_p(d_out4_ptr), C.c_void_p(d_wunique_ptr),
                                                     C.byref(n), C.c_void_p(stream)))
        return n.value

    # ---- outer boundary (batches) ------------------------------------------------------------
    def hash_batch(self, bases, offsets, ks):
        ks = _ks(ks)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        ho = np.zeros(n + 1, dtype=np.uint64)
        out = _u64p()
        _chk(self._lib.rk_hash_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), n, _p(ks, C.c_int), len(ks),
                                     C.byref(out), _p(ho, C.c_uint64)))
        tot = int(ho[-1])
        r = np.ctypeslib.as_array(out, shape=(max(tot, 1),))[:tot].copy()
        self._lib.rk_free(out)
        return r, ho

    def sketch_batch(self, bases, offsets, ks, sketch_size):
        ks = _ks(ks)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        sk = np.zeros((n, sketch_size), dtype=np.uint64)
        ln = np.zeros(n, dtype=np.int32)
        _chk(self._lib.rk_sketch_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), n, _p(ks, C.c_int), len(ks),
                                       sketch_size, _p(sk, C.c_uint64), _p(ln, C.c_int32)))
        return sk, ln

    def set_references(self, bases, offsets, ks, sketch_size, max_samples=None, counter_slots=0, count_distinct=False):
        ks = _ks(ks)
        _chk(self._lib.rk_set_reference_count_mode(self._h, 1 if count_distinct else 0))
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _chk(self._lib.rk_set_references(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), len(offsets) - 1,
                                         _p(ks, C.c_int), len(ks), sketch_size,
                                         -1 if max_samples is None else int(max_samples), counter_slots))
        self.sketch_size, self.ks = sketch_size, ks

    def set_reference_sketches(self, sketches, lens, ks, sketch_size):
        ks = _ks(ks)
        sketches = np.ascontiguousarray(sketches, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        _chk(self._lib.rk_set_reference_sketches(self._h, _p(sketches, C.c_uint64), _p(lens, C.c_int32), len(lens),
                                                 _p(ks, C.c_int), len(ks), sketch_size))
        self.sketch_size, self.ks = sketch_size, ks

    def get_reference_sketches(self):
        n = self._lib.rk_num_references(self._h)
        sk = np.zeros((n, self.sketch_size), dtype=np.uint64)
        ln = np.zeros(n, dtype=np.int32)
        _chk(self._lib.rk_get_reference_sketches(self._h, _p(sk, C.c_uint64), _p(ln, C.c_int32)))
        return sk, ln

    def set_depth_filter(self, counter, min_kmer_occ):
        _chk(self._lib.rk_set_depth_filter(self._h, counter._h if counter is not None else None, min_kmer_occ))
        self._depth = counter

    def set_min_num_bound(self, bound):
        """Row field 3 under a depth filter: exact min_num (bound < 0, default) or min(min_num, bound) -- see rkmh_amd.h."""
        _chk(self._lib.rk_set_min_num_bound(self._h, int(bound)))

    def count_batch(self, bases, offsets, counter):
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _chk(self._lib.rk_count_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), len(offsets) - 1, counter._h))

    def depth_map_tag(self, ks, bases, offsets) -> bytes:
        """Provenance tag of the read-depth map these reads produce under this context's policy (for Counter.save/load)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        kk = (C.c_int * len(ks))(*ks)
        tag = (C.c_uint8 * 128)()
        _chk(self._lib.rk_depth_map_tag(self._h, kk, len(ks), _p(bases, C.c_uint8), _p(offsets, C.c_uint64), len(offsets) - 1, tag))
        return bytes(tag)

    def classify(self, bases, offsets, out=None) -> np.ndarray:
        """main_stream's per-read loop for a host batch -> int32 [n,4] (max_id, max_shared, diff, min_num).
        Page-locked arrays (pinned_array) are read / written by DMA in place; anything else goes through staging buffers."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if out is None:
            out = np.zeros((n, 4), dtype=np.int32)
        _chk(self._lib.rk_classify_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), n, _p(out, C.c_int32)))
        return out

    def set_kmer_form(self, enable):
        """Allow (default) or forbid the k-mer-space form for the references set next."""
        _chk(self._lib.rk_set_kmer_form(self._h, 1 if enable else 0))

    def set_kmer_cache(self, path):
        """File that keeps the k-mer enumeration of the next set_references between runs (rk_set_kmer_cache); None: no cache."""
        _chk(self._lib.rk_set_kmer_cache(self._h, os.fsencode(path) if path else None))

    def kmer_cache_state(self):
        """0 none, 1 loaded, 2 enumerated and written, 3 enumerated (file not writable) -- of the last set_references"""
        return int(self._lib.rk_kmer_cache_state(self._h))

    def kmer_form(self):
        """(active, k-mers found by the enumeration): is the k-mer-space form of the fused kernel in use for these references?"""
        n = C.c_uint32()
        r = self._lib.rk_kmer_form(self._h, C.byref(n))
        _chk(min(r, 0))
        return bool(r), n.value

    def index_stats(self) -> dict:
        """What the index of the references now set was built as (rk_index_stats): counters per value form; the per-k arrays as
        lists over the k-mer sizes of the run."""
        st = IndexStats()
        st.struct_size = C.sizeof(IndexStats)
        _chk(self._lib.rk_index_stats(self._h, C.byref(st)))
        nk = len(self.ks)
        return {n: (list(getattr(st, n))[:nk] if t is not C.c_uint32 else int(getattr(st, n))) for n, t in IndexStats._fields_ if n != "struct_size"}

    def classify_groups(self, bases, offsets, argmax_refs):
        """hpv16's per-read loop: (out4 [n,4] over the first argmax_refs references, counts [n, nref - argmax_refs] of the rest)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, 4), dtype=np.int32)
        tail = np.zeros((n, max(int(self._lib.rk_num_references(self._h)) - argmax_refs, 0)), dtype=np.int32)
        _chk(self._lib.rk_classify_groups_batch(self._h, _p(bases, C.c_uint8), _p(offsets, C.c_uint64), n, argmax_refs,
                                                _p(out, C.c_int32), _p(tail, C.c_int32) if tail.size else None))
        return out, tail

    @property
    def stream(self):
        return int(self._lib.rk_ctx_stream(self._h) or 0)

    def call(self, ref_bases, ref_offsets, read_bases, read_offsets, k, window_len=100):
        """main_call's candidate records (rkmh.cpp:1772-1865): list of dicts, one per passing SNP / deletion k-mer."""
        ref_offsets = np.ascontiguousarray(ref_offsets, dtype=np.uint64)
        read_offsets = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        out = C.POINTER(CallRecord)()
        n = C.c_int64()
        _chk(self._lib.rk_call(self._h, _p(ref_bases, C.c_uint8), _p(ref_offsets, C.c_uint64), len(ref_offsets) - 1,
                               _p(read_bases, C.c_uint8), _p(read_offsets, C.c_uint64), len(read_offsets) - 1, k, window_len,
                               C.byref(out), C.byref(n)))
        recs = [dict(ref=out[i].ref, pos=out[i].pos, alt_depth=out[i].alt_depth, avg_d=out[i].avg_d, depth=out[i].depth,
                     orig=chr(out[i].orig), alt=chr(out[i].alt), kind=out[i].kind) for i in range(n.value)]
        self._lib.rk_free(out)
        return recs

    def classify_device(self, d_bases_ptr, d_offsets_ptr, nreads, d_out_ptr, max_read_len=0, stream=None):
        """Same with inputs resident in HBM (raw device pointers, e.g. torch tensors' data_ptr()).
        stream: a hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream; 0 = null stream);
        None = the context's own stream."""
        if stream is None:
            stream = self.stream
        _chk(self._lib.rk_classify_batch_device(self._h, C.c_void_p(d_bases_ptr), C.c_void_p(d_offsets_ptr), nreads,
                                                C.c_void_p(d_out_ptr), max_read_len, C.c_void_p(stream)))

    def classify_device_all(self, d_bases_ptr, d_offsets_ptr, nreads, d_out_ptr, max_read_len=0, stream=None):
        """classify_device without flagged rows: reads the fused kernel hands back are answered by the general kernels
        on the resident bases (synchronises the stream)."""
        if stream is None:
            stream = self.stream
        _chk(self._lib.rk_classify_batch_device_all(self._h, C.c_void_p(d_bases_ptr), C.c_void_p(d_offsets_ptr), nreads,
                                                    C.c_void_p(d_out_ptr), max_read_len, C.c_void_p(stream)))

    def count_device(self, d_bases_ptr, d_offsets_ptr, nreads, counter, stream=None):
        if stream is None:
            stream = self.stream
        _chk(self._lib.rk_count_batch_device(self._h, C.c_void_p(d_bases_ptr), C.c_void_p(d_offsets_ptr), nreads,
                                             counter._h, C.c_void_p(stream)))
