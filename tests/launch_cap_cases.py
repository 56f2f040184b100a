"""The inventory of launch caps: one entry per __global__ kernel of the data-plane files (FILES), read by
tests/test_launch_cap_inventory_host.py -- a kernel without an entry fails that test by name -- and by the crossing tests
of tests/test_gpu_launch_caps.py.

class:
  uncapped   grid = ceil(items / k), no loop over the grid: every size runs the same code per item;
  fixed      one block or one wave, whatever the size (a loop inside it, if any, is noted);
  capped     the grid stops growing at a constant and a loop walks the items beyond it.  `item` is what the loop walks,
             `line` the largest count that still takes ONE trip per thread / wave / block, as arithmetic on the source's
             own constants, `test` the test that runs more than that in one call.  `test` None: no test crosses the line,
             and `why` says what keeps one from it.

GRID_FOR is cv_grid_for's default geometry (csrc/cv_dev_common.hpp): 4 096 blocks of 256 threads under CV_GRID_STRIDE."""

FILES = ("cv_textparse", "cv_trainset", "cv_truth_dev", "cv_beditems_dev", "cv_bamtrain", "cv_candrows_dev", "cv_callcols_dev",
         "cv_vcf_dev", "cv_rowtext_dev", "cv_eval", "cv_inflate_dev", "cv_gzip_dev", "cv_blosc_dev", "cv_blosc_pack_dev", "cv_bam_dev",
         "cv_vcfmerge_dev", "cv_bgzf_deflate_dev")
# the compute plane: held by the oracle, parity and planted tests, whose shapes are the model's and not a launch cap's
OUTSIDE = ("cv_api", "cv_kernels_ref", "cv_kernels_mfma", "cv_kernels_wgrad", "cv_pileup", "cv_post", "cv_train")

GRID_FOR = 4096 * 256

_NEW = "tests/test_gpu_launch_caps.py::"
_BIG = "tests/test_gpu_past_4gib.py::"
_MERGE = _NEW + "test_vcf_merge_past_the_grid_stride_line"
_DEFLATE = "tests/test_gpu_bgzf_deflate.py::"


def _uncapped(file, grid):
    return {"file": file, "class": "uncapped", "grid": grid}


def _fixed(file, note):
    return {"file": file, "class": "fixed", "note": note}


def _capped(file, item, line, test, why=None, also=None):
    e = {"file": file, "class": "capped", "item": item, "line": line, "test": test}
    if why:
        e["why"] = why
    if also:
        e["also"] = also
    return e


def _grid_for(file, item, test, items_per=1, why=None):
    """a CV_GRID_STRIDE kernel behind cv_grid_for; items_per: items of the loop per counted unit (row, entry)"""
    return _capped(file, item, GRID_FOR // items_per, test, why)


KERNELS = {
    # ---- cv_textparse.hip ---------------------------------------------------------------------------------------------------
    "tp_count_newlines": _capped("cv_textparse", "4 KiB tiles of the slab (INDEX_GRID = 2048 blocks, TILE = 256 * 16 bytes)", 2048 * 4096,
                                 _NEW + "test_parse_rows_past_the_parse_line",
                                 also=["tests/test_gpu_text_parse.py::test_volume_in_the_producers_format"]),
    "tp_line_ends": _capped("cv_textparse", "4 KiB tiles of the slab (INDEX_GRID = 2048 blocks, TILE = 256 * 16 bytes)", 2048 * 4096,
                            _NEW + "test_parse_rows_past_the_parse_line",
                            also=["tests/test_gpu_text_parse.py::test_volume_in_the_producers_format"]),
    "tp_begin": _fixed("cv_textparse", "one thread"),
    "tp_parse_rows": _capped("cv_textparse", "lines, one wave each (PARSE_GRID = 2048 blocks x PARSE_WAVES = 4)", 2048 * 4,
                             _NEW + "test_parse_rows_past_the_parse_line",
                             also=["tests/test_gpu_text_parse.py::test_volume_in_the_producers_format"]),
    "tp_gather_rows": _capped("cv_textparse", "16-byte pieces, 132 per row (4096 blocks x 256 threads)", GRID_FOR // 132,
                              _BIG + "test_gather_rows_into_the_large_output"),
    "tp_token_offsets": _fixed("cv_textparse", "one workgroup of 1 024 threads walks the rows in steps of its size with a carry; 1 025 "
                               "steps in " + _NEW + "test_gather_tokens_past_the_token_copy_line"),
    "tp_token_copy": _capped("cv_textparse", "rows (4096 blocks x 256 threads, CV_GRID_STRIDE)", GRID_FOR,
                             _NEW + "test_gather_tokens_past_the_token_copy_line"),
    "tp_find_begin": _fixed("cv_textparse", "one block of CV_TEXT_FIND_MAX threads"),
    "tp_find_newline": _capped("cv_textparse", "4 KiB tiles of the text (FIND_GRID = 1024 blocks)", 1024 * 4096,
                               _BIG + "test_find_newline_either_side_of_2_32_bytes"),
    "tp_run_flags": _grid_for("cv_textparse", "lines + 1", _NEW + "test_item_lines_past_the_grid_stride_line"),
    # ---- cv_trainset.hip ----------------------------------------------------------------------------------------------------
    "ts_tokens": _grid_for("cv_trainset", "rows", _NEW + "test_trainset_tokens_past_the_grid_stride_line"),
    "ts_run_index": _grid_for("cv_trainset", "rows", _NEW + "test_trainset_tokens_past_the_grid_stride_line"),
    "ts_join": _grid_for("cv_trainset", "rows", _NEW + "test_trainset_join_past_the_grid_stride_line"),
    "ts_keys": _grid_for("cv_trainset", "rows", _NEW + "test_trainset_finish_past_the_grid_stride_line"),
    "ts_heads": _grid_for("cv_trainset", "rows + 1", _NEW + "test_trainset_finish_past_the_grid_stride_line"),
    "ts_entries": _grid_for("cv_trainset", "rows", _NEW + "test_trainset_finish_past_the_grid_stride_line"),
    "ts_labels": _grid_for("cv_trainset", "entries * 16 labels", _NEW + "test_trainset_finish_past_the_grid_stride_line", items_per=16),
    "ts_zero_total": _fixed("cv_trainset", "one thread"),
    "ts_gather": _grid_for("cv_trainset", "rows * 136 16-byte pieces (132 of the row, 4 of the label)",
                           _NEW + "test_trainset_gather_past_the_grid_stride_line", items_per=136),
    # ---- cv_truth_dev.hip ---------------------------------------------------------------------------------------------------
    "tl_verdicts": _grid_for("cv_truth_dev", "max_lines + 1", _NEW + "test_truth_lines_past_the_grid_stride_line"),
    "tl_rows": _grid_for("cv_truth_dev", "lines", _NEW + "test_truth_lines_past_the_grid_stride_line"),
    "bt_end_keys": _grid_for("cv_truth_dev", "intervals", _NEW + "test_bed_table_past_the_grid_stride_line"),
    "bt_begin_keys": _grid_for("cv_truth_dev", "intervals", _NEW + "test_bed_table_past_the_grid_stride_line"),
    "bt_gather": _grid_for("cv_truth_dev", "intervals", _NEW + "test_bed_table_past_the_grid_stride_line"),
    "bt_finish": _grid_for("cv_truth_dev", "intervals, then contigs + 1 (at most 65 536: its second loop never strides; "
                           "test_three_rows_over_65535_contigs runs it over more offsets than rows)",
                           _NEW + "test_bed_table_past_the_grid_stride_line"),
    "tt_keys": _grid_for("cv_truth_dev", "truth rows", _NEW + "test_truth_tables_past_the_grid_stride_line"),
    "tt_tails": _grid_for("cv_truth_dev", "truth rows + 1", _NEW + "test_truth_tables_past_the_grid_stride_line"),
    "tt_emit": _grid_for("cv_truth_dev", "truth rows, then contigs + 1 (as bt_finish)", _NEW + "test_truth_tables_past_the_grid_stride_line"),
    # ---- cv_beditems_dev.hip ------------------------------------------------------------------------------------------------
    "il_verdicts": _grid_for("cv_beditems_dev", "max_lines + 1", _NEW + "test_item_lines_past_the_grid_stride_line"),
    "il_rows": _grid_for("cv_beditems_dev", "lines", _NEW + "test_item_lines_past_the_grid_stride_line"),
    "ik_flags": _grid_for("cv_beditems_dev", "rows + 1", _NEW + "test_items_keep_counts_past_the_grid_stride_line"),
    "ik_copy": _capped("cv_beditems_dev", "rows, one wave each (65 536 blocks x 4 waves)", 65536 * 4,
                       _NEW + "test_items_keep_text_past_the_copy_line"),
    "sp_flags": _grid_for("cv_beditems_dev", "positions + 1", _NEW + "test_sample_positions_past_the_grid_stride_line"),
    "sp_emit": _grid_for("cv_beditems_dev", "positions", _NEW + "test_sample_positions_past_the_grid_stride_line"),
    # ---- cv_bamtrain.hip ----------------------------------------------------------------------------------------------------
    "bt_columns": _grid_for("cv_bamtrain", "centres of the pileup handle", None,
                            why="the centres are the handle's own (cv_pileup_set_candidates), and installing n centres allocates the "
                                "handle's counters, n * 33 * 9 * 4 bytes in one buffer (install_alloc, cv_pileup.hip): (GRID_FOR + 1) * "
                                "1 188 = 1 245 709 476 bytes, past the 512 MB a test may allocate."),
    "bt_pair_count": _grid_for("cv_bamtrain", "rows", _NEW + "test_bamtrain_pair_past_the_grid_stride_line"),
    "bt_pair_keep": _grid_for("cv_bamtrain", "rows", _NEW + "test_bamtrain_pair_past_the_grid_stride_line"),
    # ---- cv_candrows_dev.hip ------------------------------------------------------------------------------------------------
    "candorder_flag": _grid_for("cv_candrows_dev", "entries + 1", _NEW + "test_candidate_order_and_rows_past_the_grid_stride_line"),
    "candorder_place": _grid_for("cv_candrows_dev", "entries", _NEW + "test_candidate_order_and_rows_past_the_grid_stride_line"),
    "candrows_len": _grid_for("cv_candrows_dev", "rows + 1", _NEW + "test_candidate_order_and_rows_past_the_grid_stride_line"),
    "candrows_write": _uncapped("cv_candrows_dev", "ceil(rows / 64) one-wave blocks"),
    # ---- cv_callcols_dev.hip, cv_vcf_dev.hip, cv_rowtext_dev.hip --------------------------------------------------------------
    "cc_verdict": _uncapped("cv_callcols_dev", "ceil((n + 1) / 256)"),
    "cc_write": _uncapped("cv_callcols_dev", "ceil(n / 16): 16 lanes per centre"),
    "vcf_len": _uncapped("cv_vcf_dev", "ceil((n + 1) / 256)"),
    "vcf_write": _uncapped("cv_vcf_dev", "ceil(n / 256)"),
    "rowtext_len": _uncapped("cv_rowtext_dev", "ceil((rows + 1) / 4): one wave per row"),
    "rowtext_write": _uncapped("cv_rowtext_dev", "ceil(rows / 4): one wave per row"),
    # ---- cv_eval.hip, cv_inflate_dev.hip ----------------------------------------------------------------------------------------
    "eval_counts": _capped("cv_eval", "candidates (EV_GRID = 256 blocks x EV_THREADS = 256)", 256 * 256,
                           "tests/test_gpu_eval.py::test_kernel_counts_match_the_host_report"),
    "bgzf_inflate": _capped("cv_inflate_dev", "members, one wave each (INFLATE_GRID = 4096 blocks x INFLATE_WAVES = 4)", 4096 * 4,
                            "tests/test_gpu_bgzf.py::test_many_members_in_one_call"),
    # ---- cv_gzip_dev.hip ----------------------------------------------------------------------------------------------------
    "gzip_find": _capped("cv_gzip_dev", "guesses, one wave each (GRID = 4096 blocks x WAVES = 4)", 4096 * 4,
                         _NEW + "test_one_gzip_slab_past_the_find_and_decode_lines"),
    "gzip_decode": _capped("cv_gzip_dev", "chunks, one wave each (GRID = 4096 blocks x WAVES = 4)", 4096 * 4,
                           _NEW + "test_one_gzip_slab_past_the_find_and_decode_lines"),
    "gzip_tails": _fixed("cv_gzip_dev", "one block of 1 024 threads walks the chunks in order"),
    "gzip_rest": _capped("cv_gzip_dev", "symbols (GRID = 4096 blocks of 256 threads, the grid sized for 8 symbols per thread: a thread "
                         "makes several trips from 257 symbols on, the grid stops growing here); it writes what a chunk holds in "
                         "front of its last 32 KiB", 4096 * 256 * 8, _NEW + "test_gzip_resolve_past_the_rest_line"),
    "gzip_crc": _capped("cv_gzip_dev", "1 KiB pieces of the text (GRID = 4096 blocks x 256 threads, CRC_CHUNK = 1024)", 4096 * 256, None,
                        why="4096 * 256 pieces of 1 024 bytes are 2^30 bytes of text in one buffer: past the 512 MB a test may "
                            "allocate.  The pieces are independent (each register starts from 0)."),
    # ---- cv_blosc_dev.hip, cv_blosc_pack_dev.hip ------------------------------------------------------------------------------------
    "blosc_decode": _capped("cv_blosc_dev", "streams, one wave each (DECODE_GRID = 8192 blocks x DECODE_WAVES = 4)", 8192 * 4,
                            _NEW + "test_blosc_streams_past_the_decode_line"),
    "blosc_unpack": _uncapped("cv_blosc_dev", "(slices of 16 KiB, chunks): at most 65 535 chunks per call"),
    "pack_encode": _capped("cv_blosc_pack_dev", "streams, one one-wave block each (MAX_GRID = 2^20)", 1 << 20,
                           _NEW + "test_blosc_pack_past_the_stream_line"),
    "pack_layout": _uncapped("cv_blosc_pack_dev", "one block per chunk (at most 65 535)"),
    "pack_offsets": _fixed("cv_blosc_pack_dev", "one block of 256 threads scans the chunk totals"),
    "pack_assemble": _capped("cv_blosc_pack_dev", "streams, one block each (MAX_GRID = 2^20)", 1 << 20,
                             _NEW + "test_blosc_pack_past_the_stream_line"),
    # ---- cv_bam_dev.hip -----------------------------------------------------------------------------------------------------
    "bam_walk": _uncapped("cv_bam_dev", "ceil(walkers / 64), one thread per walker"),
    "bam_gather": _capped("cv_bam_dev", "walkers (the slab's start and the linear-index entries that point into it), one block each "
                          "(4096 blocks)", 4096, _NEW + "test_one_bam_slab_past_the_walker_line"),
    "bam_count": _uncapped("cv_bam_dev", "ceil(records / 256)"),
    "bam_split": _uncapped("cv_bam_dev", "ceil(records / 256)"),
    "bam_heads": _uncapped("cv_bam_dev", "ceil(records / 256)"),
    "bam_resolve": _uncapped("cv_bam_dev", "ceil(records / 256); a ballot per wave, no loop in front of it"),
    "bam_totals": _fixed("cv_bam_dev", "one thread"),
    "bam_emit": _uncapped("cv_bam_dev", "ceil(records / 4): one wave per record"),
    # ---- cv_vcfmerge_dev.hip -------------------------------------------------------------------------------------------------
    "vm_fields": _grid_for("cv_vcfmerge_dev", "records", _MERGE),
    "vm_sorted": _grid_for("cv_vcfmerge_dev", "records + 1", _MERGE),
    "vm_gather": _capped("cv_vcfmerge_dev", "tiles of 64 output records, one one-wave block each (65 536 blocks; the block's LDS tile "
                         "serves its second tile)", 65536 * 64, _NEW + "test_vcf_gather_past_the_tile_line"),
    "vm_heads": _grid_for("cv_vcfmerge_dev", "records + 1", _MERGE),
    "vm_chunks": _grid_for("cv_vcfmerge_dev", "records", _MERGE),
    "vm_chunk_out": _grid_for("cv_vcfmerge_dev", "records", _MERGE),
    "vw_fill": _grid_for("cv_vcfmerge_dev", "windows of 16 384 bases", _MERGE),
    "vw_min": _grid_for("cv_vcfmerge_dev", "records", _MERGE),
    "vw_backfill": _capped("cv_vcfmerge_dev", "contig ranks, one block each (1 024 blocks)", 1024, _MERGE),
    # ---- cv_bgzf_deflate_dev.hip ---------------------------------------------------------------------------------------------
    "bd_compress": _capped("cv_bgzf_deflate_dev", "members, one workgroup each (MAX_GRID = 512; the workgroup's LDS state and its "
                           "verdicts in the workspace serve its second member)", 512,
                           _DEFLATE + "test_multi_tile_members_past_the_workgroup_line",
                           also=[_DEFLATE + "test_more_members_than_workgroups"]),
    "bd_offsets": _fixed("cv_bgzf_deflate_dev", "one block of 256 threads walks the sizes in steps of its size with a carry; 20 steps in "
                         + _DEFLATE + "test_more_members_than_workgroups"),
    "bd_assemble": _capped("cv_bgzf_deflate_dev", "members, one block each (4 096 blocks)", 4096,
                           _DEFLATE + "test_more_members_than_workgroups"),
}
