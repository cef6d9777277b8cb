"""tools/device_code_diff.py on hand-written assembly: what counts as a kernel's instruction text, and the three verdicts."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('device_code_diff', os.path.join(ROOT, 'tools', 'device_code_diff.py'))
dcd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(dcd)

ASM = """
	.text
	.globl	_Z1kPf
_Z1kPf:                                 ; @_Z1kPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0   ; comment
	s_cbranch_scc1 .LBB{n}_2
.LBB{n}_1:
	{first}
	{second}
.LBB{n}_2:
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel _Z1kPf
		.amdhsa_kernarg_size {kernarg}
		.amdhsa_next_free_vgpr {vgpr}
	.end_amdhsa_kernel
	.text
.Lfunc_end{n}:
"""
REMARKS = """x.hip:1:1: remark: Function Name: _Z1kPf [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     TotalSGPRs: 10 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs: {vgpr} [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
"""


def kernel(n=0, first='v_mov_b32_e32 v0, 1', second='v_add_f32_e32 v1, v0, v0', kernarg=8, vgpr=2):
    k = dcd.parse_asm(ASM.format(n=n, first=first, second=second, kernarg=kernarg, vgpr=vgpr))
    assert list(k) == ['_Z1kPf']
    k['_Z1kPf']['remarks'] = dcd.parse_remarks(REMARKS.format(vgpr=vgpr))['_Z1kPf']
    return k['_Z1kPf']


def test_instruction_text_is_label_to_descriptor_without_comments_and_with_renamed_labels():
    k = kernel(n=7)
    assert k['lines'] == ['s_load_dwordx2 s[0:1], s[4:5], 0x0', 's_cbranch_scc1 .L0', '.L1:', 'v_mov_b32_e32 v0, 1',
                          'v_add_f32_e32 v1, v0, v0', '.L0:', 's_endpgm']
    assert dcd.n_instructions(k['lines']) == 5
    assert k['desc'] == {'.amdhsa_next_free_vgpr': '2'}                 # the kernarg size is not compared
    assert k['remarks'] == {'TotalSGPRs': '10', 'VGPRs': '2', 'ScratchSize [bytes/lane]': '0', 'Occupancy [waves/SIMD]': '8'}


def test_verdicts():
    base = kernel()
    assert dcd.classify(base, kernel(n=3, kernarg=16)) == 'identical'   # other label numbers, other kernarg size
    assert dcd.classify(base, kernel(first='v_mov_b32_e32 v0, 2')) == 'permuted'          # an operand
    assert dcd.classify(base, kernel(first='v_add_f32_e32 v1, v0, v0', second='v_mov_b32_e32 v0, 1')) == 'permuted'   # order
    assert dcd.classify(base, kernel(first='v_mul_f32_e32 v0, v0, v0')) == 'moved'        # another opcode
    assert dcd.classify(base, kernel(vgpr=3)) == 'moved'                                  # same text, other resources


def test_symbols_are_matched_across_units_and_copies_collapse():
    a = {'_Z1kPf': {'u1': kernel(), 'u2': kernel()}, '_Z4gonev': {'u1': kernel()}}
    b = {'_Z1kPf': {'u3': kernel(n=5)}, '_Z3newv': {'u3': kernel()}}
    rows = {r['symbol']: r for r in dcd.compare(a, b)}
    assert rows['_Z1kPf']['status'] == 'identical' and rows['_Z1kPf']['units_a'] == ['u1', 'u2'] and rows['_Z1kPf']['units_b'] == ['u3']
    assert rows['_Z4gonev']['status'] == 'only in A' and rows['_Z3newv']['status'] == 'only in B'
    b['_Z1kPf']['u3'] = kernel(vgpr=4)
    assert {r['symbol']: r for r in dcd.compare(a, b)}['_Z1kPf']['status'] == 'moved'
