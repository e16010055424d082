"""Every source file that chooses between two access-mode instances of a kernel names the tests that run both.

Two options pick a compiled copy at launch time: ``blas1_nt`` through stream_nt() / block_nt() (common.hpp, block.hip), and
``nontemporal`` through reads of the context's opt_nt.  The default of the first switches at 6 * 2^20 rows, the default of
the second is 1 -- so a suite of small shapes runs one instance of each unless a test sets the option.  This file scans
stormruler_amd/csrc for the launch sites and holds each file that has one to an entry of LEDGER: (test file, test function)
pairs that run BOTH instances against a reference.  A new kernel family with an access-mode instance fails here until someone
names the test.  (It checks that the named tests exist, not what they assert; nothing here needs a GPU.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stormruler_amd", "csrc")

MODES_FILE = "test_gpu_access_modes.py"  # all four (nontemporal, blas1_nt) modes, bitwise; the owning files' pins in (0, 2)

LEDGER = {
    # test_gpu_exact_statements.py, test_gpu_exact_reductions.py: blas1_nt 0 and 2 at every size, and 1 at the switch itself
    "blas1.hip": [("test_gpu_exact_statements.py", "test_every_statement_is_exact_on_integer_data"),
                  ("test_gpu_exact_statements.py", "test_every_loop_is_exact_beyond_one_trip_of_the_grid"),
                  ("test_gpu_exact_reductions.py", "test_blas1_reductions_are_exact")],
    # test_gpu_exact_statements.py: the held-back statements (lazy_lin_kernel) under blas1_nt 0 and 2
    "lazy.hip": [("test_gpu_exact_statements.py", "test_every_statement_is_exact_on_integer_data"),
                 ("test_gpu_exact_statements.py", "test_the_cg_update_pair_and_its_sum_are_exact")],
    # test_gpu_parity.py, test_gpu_cross_product.py: nontemporal 0 and 1 on every record format
    "spmv_sell.hip": [("test_gpu_parity.py", "test_spmv_kernel_variants_agree"),
                      ("test_gpu_cross_product.py", "test_launch_shaping_knobs_do_not_change_results")],
    # test_gpu_block.py: nontemporal 0 and 1, k = 1 .. 8
    "spmv_block.hip": [("test_gpu_block.py", "test_mul_block_equals_the_single_apply_bit_for_bit")],
    # the fused loops: the exact pins under blas1_nt 2 beside the default; test_gpu_streaming_modes.py: 0 against 2, bitwise
    "solver_fused.hip": [("test_gpu_exact_steps.py", "test_cg_steps_non_temporal"),
                         ("test_gpu_exact_steps.py", "test_bicgstab_steps_non_temporal"),
                         ("test_gpu_streaming_modes.py", "test_nontemporal_and_plain_streaming_give_bitwise_equal_solves")],
    "solver_cg.hip": [("test_gpu_exact_steps.py", "test_cg_steps_non_temporal"), ("test_gpu_exact_steps.py", "test_cg_steps"),
                      ("test_gpu_streaming_modes.py", "test_nontemporal_and_plain_streaming_give_bitwise_equal_solves")],
    "solver_bicgstab.hip": [("test_gpu_exact_steps.py", "test_bicgstab_steps_non_temporal"),
                            ("test_gpu_exact_steps.py", "test_bicgstab_steps"),
                            ("test_gpu_streaming_modes.py", "test_nontemporal_and_plain_streaming_give_bitwise_equal_solves")],
    # the rows steps2 / steps3 / steps4 / step / cgs2 and their -nt twins (blas1_nt 2) against the same GmresPins
    "solver_gmres.hip": [("test_gpu_exact_gmres.py", "test_gmres_against_the_exact_reference"),
                         ("test_gpu_streaming_modes.py", "test_nontemporal_and_plain_streaming_give_bitwise_equal_solves")],
    # Engine::stream_flags: the flag of every krylov_device.hpp kernel (lin_kernel, lin2_kernel, the lin_dot / pre_dots bodies,
    # fd_shift_kernel, fd_diff_body).  ENGINE_CONFIGS with blas1_nt 2, the Jacobi-preconditioned solves, the JFNK product
    "krylov_engine.hpp": [("test_gpu_exact_first_step.py", "test_engine_methods_against_the_exact_reference"),
                          ("test_gpu_exact_first_step.py", "test_engine_methods_with_jacobi"),
                          ("test_gpu_exact_first_step.py", "test_engine_methods_with_jacobi_non_temporal"),
                          ("test_gpu_exact_steps.py", "test_cg_steps_non_temporal"),
                          (MODES_FILE, "test_finite_difference_product_streams_non_temporally"),
                          (MODES_FILE, "test_newton_solve_is_the_same_in_every_mode")],
    "precond_cheb.hip": [(MODES_FILE, "test_chebyshev_apply_in_every_mode"),
                         (MODES_FILE, "test_chebyshev_closed_form_in_the_last_mode")],
    "amg.hip": [(MODES_FILE, "test_multigrid_cycle_with_the_chebyshev_smoother_in_every_mode"),
                (MODES_FILE, "test_multigrid_cycle_against_the_restatement_in_the_last_mode"),
                (MODES_FILE, "test_multigrid_cycle_with_the_jacobi_smoother_in_every_mode"),
                (MODES_FILE, "test_a_jacobi_sweep_is_exact_on_integers_in_the_last_mode"),
                (MODES_FILE, "test_projection_is_exact_on_integers_in_the_last_mode"),
                (MODES_FILE, "test_null_space_object_in_every_mode")],
    "op_update.hip": [(MODES_FILE, "test_face_weight_refresh_in_both_streaming_modes"),
                      (MODES_FILE, "test_refreshed_integer_weights_apply_exactly")],
    "op_reduced.hip": [(MODES_FILE, "test_reduced_apply_with_plain_loads"),
                       (MODES_FILE, "test_face_weight_refresh_in_both_streaming_modes")],
    "block.hip": [(MODES_FILE, "test_one_column_block_kernels_in_both_streaming_modes"),
                  (MODES_FILE, "test_one_column_block_cg_against_the_exact_pins")],
}

SITE = re.compile(r"\bstream_nt\s*\(|\bblock_nt\s*\(|\bopt_nt\b")
# not launch sites: the two functions' definitions, the field's declaration, the option parser's assignment
NOT_A_SITE = re.compile(r"static\s+inline\s+int\s+(stream_nt|block_nt)\s*\(|\bint64_t\s+opt_nt\s*=|\bopt_nt\s*=\s*value\b")


def _code(text):
    """The text without its comments (a comment may name stream_nt() without calling it)."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def launch_sites():
    """{file name: [line numbers]} of the access-mode choices under stormruler_amd/csrc."""
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            lines = _code(f.read()).split("\n")
        hits = []
        for k, line in enumerate(lines, 1):
            rest = NOT_A_SITE.sub("", line)  # (block_nt's definition line also CALLS stream_nt: that call stays a site)
            if SITE.search(rest):
                hits.append(k)
        if hits:
            found[name] = hits
    return found


def test_the_scan_finds_the_known_sites():
    """The scan itself: the definitions and the parser are not sites, the known families are."""
    sites = launch_sites()
    assert "common.hpp" not in sites and "context.hip" not in sites and "blas1_device.hpp" not in sites, sites
    for name in ("blas1.hip", "precond_cheb.hip", "amg.hip", "op_update.hip", "block.hip", "krylov_engine.hpp", "spmv_sell.hip"):
        assert name in sites, name
    assert len(sites["block.hip"]) >= 4  # block_nt's own call of stream_nt and its three callers


def test_every_file_with_an_access_mode_choice_is_in_the_ledger():
    sites = launch_sites()
    missing = sorted(set(sites) - set(LEDGER))
    assert not missing, f"no test named for the access-mode instances chosen in {missing} (lines {[sites[m] for m in missing]})"
    stale = sorted(set(LEDGER) - set(sites))
    assert not stale, f"LEDGER names files without an access-mode choice: {stale}"


def test_every_ledger_entry_names_an_existing_test():
    for name, entries in LEDGER.items():
        assert entries, name
        for test_file, function in entries:
            path = os.path.join(ROOT, "tests", test_file)
            assert os.path.exists(path), (name, test_file)
            with open(path) as f:
                assert re.search(rf"^def {re.escape(function)}\(", f.read(), flags=re.M), (name, test_file, function)
