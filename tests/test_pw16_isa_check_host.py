"""tools/check_pw16_isa.py (run by the build on conv_pw16.hip's ISA) on canned listings: it rejects a buffer access inside a loop closed
by s_cbranch_execnz (the waterfall hipcc builds around a descriptor it cannot prove wave-uniform) and accepts the same accesses in
straight code, in a scalar loop, and in an out-of-line block that branches back into earlier code."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = '_ZN3csd11pw16_kernelILi2ELi2ELi2ELb1ELb0ELb0EEEvPKfS2_PKcNS_7PwKArgsE'


def _checker():
    spec = importlib.util.spec_from_file_location('check_pw16_isa', os.path.join(ROOT, 'tools', 'check_pw16_isa.py'))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    return chk


WATERFALL = [
    '.LBB0_4:                                ; =>This Inner Loop Header: Depth=2',
    '\tv_readfirstlane_b32 s8, v10',
    '\tv_readfirstlane_b32 s9, v11',
    '\tv_readfirstlane_b32 s10, v12',
    '\tv_readfirstlane_b32 s11, v13',
    '\tv_cmp_eq_u64_e32 vcc, s[8:9], v[10:11]',
    '\tv_cmp_eq_u64_e64 s[0:1], s[10:11], v[12:13]',
    '\ts_and_b64 s[0:1], vcc, s[0:1]',
    '\ts_and_saveexec_b64 s[0:1], s[0:1]',
    '\tbuffer_store_dwordx4 v[2:5], v6, s[8:11], 0 offen',
    '\ts_xor_b64 exec, exec, s[0:1]',
    '\ts_cbranch_execnz .LBB0_4',
]
STRAIGHT = ['\tbuffer_store_dwordx4 v[2:5], v6, s[8:11], 0 offen']


def _kernel(body, name=NAME):
    head = ['\t.text', name + ':                       ; @' + name, '; %bb.0:', '\ts_load_dwordx4 s[8:11], s[0:1], 0x0',
            '.LBB0_2:                                ; =>This Loop Header: Depth=1',
            '\tglobal_load_dwordx4 v[2:5], v[0:1], off', '\ts_waitcnt vmcnt(0)',
            '\tv_mfma_f32_16x16x32_f16 v[2:5], v[20:23], v[24:27], v[2:5]']
    tail = ['\ts_add_i32 s2, s2, 1', '\ts_cmp_lt_i32 s2, s3', '\ts_cbranch_scc1 .LBB0_2', '; %bb.9:', '\ts_endpgm', '\t.section\t.rodata']
    return head + body + tail


def test_pw16_isa_check_rejects_a_waterfall_and_accepts_uniform_code(tmp_path):
    chk = _checker()
    # an out-of-line block (placed behind the loop) that rejoins the loop body through s_cbranch_execnz: a backward branch, no loop
    rejoin = (_kernel(['\ts_cbranch_vccnz .LBB0_7', '.LBB0_5:'] + STRAIGHT)[:-3]
              + ['\ts_branch .LBB0_9', '.LBB0_7:', '\tbuffer_store_dwordx4 v[2:5], v7, s[8:11], 0 offen', '\ts_cbranch_execnz .LBB0_5',
                 '.LBB0_9:', '\ts_endpgm'])
    # the waterfall in a kernel the check is not about
    other = _kernel(WATERFALL, name='_ZN3csd13tapsum_kernelILi3EEEvPKfS2_S2_Pfiiiifi') + _kernel(STRAIGHT)
    for lines, rc in ((_kernel(WATERFALL), 1), (_kernel(STRAIGHT), 0), (rejoin, 0), (other, 0), (_kernel(STRAIGHT) + _kernel(WATERFALL, NAME.replace('Lb0ELb0E', 'Lb1ELb0E')), 1),
                      (['\t.text', '\ts_endpgm'], 1)):          # no pw16_kernel at all: an error, not a pass
        p = tmp_path / 'k.s'
        p.write_text('\n'.join(lines) + '\n')
        assert chk.main(str(p)) == rc, lines
    built = os.path.join(ROOT, 'conditional_score_diffusion_amd', 'csrc', 'conv_pw16.s')
    if os.path.exists(built):                        # the ISA the in-tree library was built from
        assert chk.main(built) == 0
