"""tools/kernel_asm_diff.py on synthetic assembly: pairing through --rename, the kernel's own symbol
as a placeholder, and the kernarg-size rule.  No compiler and no GPU."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_asm_diff", os.path.join(REPO, "tools", "kernel_asm_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


kad = _tool()


def _asm(symbol: str, kernarg: int, add: str = "v_add_f32_e32 v1, v0, v0") -> str:
    """One kernel as hipcc -S lays it out: section, label, code, end label, descriptor."""
    return f"""\t.text
\t.section\t.text.{symbol},"axG",@progbits,{symbol},comdat
\t.protected\t{symbol}
\t.globl\t{symbol}
\t.type\t{symbol},@function
{symbol}:                                ; @{symbol}
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\t{add}
.LBB7_1:                                ; =>This Inner Loop Header
\ts_cbranch_scc1 .LBB7_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {symbol}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_kernarg_size {kernarg}
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.section\t.text.{symbol},"axG",@progbits,{symbol},comdat
.Lfunc_end7:
\t.size\t{symbol}, .Lfunc_end7-{symbol}
"""


def _compare(asm_a: str, asm_b: str, renames=()):
    ka, kb = kad.split_kernels(asm_a), kad.split_kernels(asm_b)
    # the synthetic symbols stand for their own demangled names
    recs = kad.compare_kernels(ka, kb, {k: k for k in ka}, {k: k for k in kb}, kad.parse_renames(list(renames)))
    return {r["name"].split("  (A:")[0]: r for r in recs}


RENAME = (r"old_(\w+)_kernel=new_kernel_\1",)


def test_renamed_kernel_with_identical_body_pairs_as_identical():
    recs = _compare(_asm("old_metric_kernel", 144), _asm("new_kernel_metric", 144), RENAME)
    assert list(recs) == ["new_kernel_metric"]
    assert recs["new_kernel_metric"]["status"] == "identical" and recs["new_kernel_metric"]["renamed"]


def test_without_the_rule_the_kernels_do_not_pair():
    recs = _compare(_asm("old_metric_kernel", 144), _asm("new_kernel_metric", 144))
    assert {n: r["status"] for n, r in recs.items()} == {"old_metric_kernel": "only in A", "new_kernel_metric": "only in B"}


def test_one_changed_instruction_is_a_difference():
    changed = _asm("new_kernel_metric", 144, add="v_add_f32_e32 v1, v0, v1")
    assert _compare(_asm("old_metric_kernel", 144), changed, RENAME)["new_kernel_metric"]["status"] == "differing"
    assert _compare(_asm("same_kernel", 144), _asm("same_kernel", 144, add="v_add_f32_e32 v1, v0, v1"))["same_kernel"]["status"] == "differing"


def test_kernarg_size_alone_counts_only_for_an_unrenamed_pair():
    r = _compare(_asm("old_metric_kernel", 144), _asm("new_kernel_metric", 160), RENAME)["new_kernel_metric"]
    assert r["status"] == "identical" and r["kernarg"] == ("144", "160")
    r = _compare(_asm("same_kernel", 144), _asm("same_kernel", 160), RENAME)["same_kernel"]
    assert r["status"] == "differing" and not r["renamed"]


def test_every_other_descriptor_line_still_counts_for_a_renamed_pair():
    b = _asm("new_kernel_metric", 160).replace(".amdhsa_next_free_vgpr 2", ".amdhsa_next_free_vgpr 3")
    assert _compare(_asm("old_metric_kernel", 144), b, RENAME)["new_kernel_metric"]["status"] == "differing"
