"""CPU-only: the contract of the conv routing unit, swept under the host sanitizers.  echoscene_amd/csrc/es_conv_route.hip is plain
C++ (no HIP header, no hip* call): it is compiled here with g++ -x c++ together with tests/c/conv_route_sweep.cpp -- a stand-alone
program with its own main -- under -fsanitize=address,undefined, and run.  The program asserts, for every accepted route of ~19 M
argument sets x option settings, what the planner and the workspace contract of echoscene_hip.h rely on: the slab caps (16 for
small outputs, else 8; an explicit splitk; none without a workspace), S / slabs / reduction consistent, a launchable grid, a kernel
named unless the tools' forcing options are set, chunked launches with 1 <= omax < O.  A compile failure fails the test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_route_contract_sweep_under_host_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'echoscene_amd', 'csrc')
    exe = str(tmp_path / 'conv_route_sweep')
    # (the sanitizer runtimes linked statically: the program then does not depend on the order in which shared libraries load)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-static-libasan', '-static-libubsan',
                           '-I', os.path.join(ROOT, 'include'), '-x', 'c++', os.path.join(csrc, 'es_conv_route.hip'),
                           os.path.join(ROOT, 'tests', 'c', 'conv_route_sweep.cpp'), '-o', exe])
    env = {k: v for k, v in os.environ.items() if k not in ('ES_CONV_A3', 'ES_CONV_LINWS', 'ES_CONV_N16')}      # (the defaults' routes)
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert p.returncode == 0, 'exit %d\n%s\n%s' % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert ' 0 violations' in p.stdout, p.stdout
