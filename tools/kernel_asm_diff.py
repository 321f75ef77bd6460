"""Which kernels did a change touch?  Compares two device assembly listings of one source file kernel by kernel:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S es_vol.hip -o new.s      (and the same on the parent's sources)
    python tools/kernel_asm_diff.py parent.s new.s

Per `.amdhsa_kernel` symbol the text from the symbol's label to its `.Lfunc_end` (instructions and the kernel descriptor with its
register counts), comments stripped and the function index in local labels normalised, is hashed.  Prints how many kernels are
identical under the same symbol, names the ones that differ or went, and lists the new ones with their register and spill counts
(profiles/conv_route_split_notes.md describes the method; profiles/up_fold_notes.md uses it).  CPU only.

    python tools/kernel_asm_diff.py parent.s new.s --rename '(anonymous namespace)::ConvGeom=ConvGeom'

compares under the DEMANGLED names after replacing OLD by NEW in the parent's: for a change that moves a kernel parameter's type to
another namespace, which respells the symbols of the kernels that take it and nothing else (profiles/conv_route_unit_notes.md).

    python tools/kernel_asm_diff.py parent.s new.s --table

prints, instead of the DIFFERS lines, one markdown row per differing kernel with parent -> new of: VGPRs, SGPRs, VGPR / SGPR spills,
scratch bytes, v_mfma, LDS-DMA loads (buffer_load ... lds), waterfall loops (s_cbranch_execnz: a buffer instruction whose descriptor or
soffset the compiler could not keep scalar), static LDS bytes and instructions (profiles/conv_gather_notes.md)."""
import re, sys, hashlib, subprocess


def kernels(path):
    txt = open(path).read()
    names = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', txt, re.M)
    out, meta, count = {}, {}, {}
    for n in names:
        m = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end(\d+):' % re.escape(n), txt, re.M | re.S)
        body = m.group(1)
        idx = m.group(2)
        lines = []
        for ln in body.split('\n'):
            ln = ln.split(';')[0].rstrip()
            if not ln.strip():
                continue
            ln = re.sub(r'\.LBB%s_' % idx, '.LBB_', ln)
            ln = re.sub(r'\.Ltmp\d+', '.Ltmp', ln)
            lines.append(ln)
        lines = [ln.replace(n, 'SELF') for ln in lines]
        out[n] = hashlib.sha1('\n'.join(lines).encode()).hexdigest()
        count[n] = dict(mfma=sum('v_mfma' in ln for ln in lines), dma=sum('buffer_load' in ln and ' lds' in ln for ln in lines),
                        waterfall=sum('s_cbranch_execnz' in ln for ln in lines),
                        insts=sum(ln.startswith('\t') and not ln.strip().startswith('.') for ln in lines))
        k = re.search(r'\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel' % re.escape(n), txt, re.S).group(1)
        meta[n] = dict(vgpr=re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', k).group(1), accum=re.search(r'\.amdhsa_accum_offset\s+(\d+)', k).group(1))
    # spills from the metadata
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', txt, re.S):
        n = m.group(1)
        if n in meta:
            for key in ('vgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'agpr_count', 'sgpr_count'):
                mm = re.search(r'\.%s:\s+(\d+)' % key, m.group(2))
                if mm:
                    meta[n][key] = mm.group(1)
    at = txt.find('amdhsa.kernels:')                                           # (a listing without the metadata block: no LDS column)
    for blk in (txt[at:].split('\n  - ')[1:] if at >= 0 else []):               # (.group_segment_fixed_size stands in front of .name)
        nm, lds = re.search(r'^    \.name:\s+(\S+)', blk, re.M), re.search(r'^    \.group_segment_fixed_size:\s+(\d+)', blk, re.M)
        if nm and lds and nm.group(1) in meta:
            meta[nm.group(1)]['lds'] = lds.group(1)
    for n in meta:
        meta[n].update(count[n])
    return out, meta


a, ma = kernels(sys.argv[1])
b, mb = kernels(sys.argv[2])
dem = lambda n: subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()
if '--rename' in sys.argv:
    old, new = sys.argv[sys.argv.index('--rename') + 1].split('=')
    a = {dem(n).replace(old, new): h for n, h in a.items()}
    b, mb = {dem(n): h for n, h in b.items()}, {dem(n): m for n, m in mb.items()}
    dem = lambda n: n
same = [n for n in a if n in b and a[n] == b[n]]
diff = [n for n in a if n in b and a[n] != b[n]]
print('parent kernels %d, new kernels %d, identical under the same symbol %d' % (len(a), len(b), len(same)))
if '--table' in sys.argv:
    keys = [('vgpr_count', 'VGPRs'), ('sgpr_count', 'SGPRs'), ('vgpr_spill_count', 'VGPR spills'), ('sgpr_spill_count', 'SGPR spills'),
            ('private_segment_fixed_size', 'scratch B'), ('mfma', 'v_mfma'), ('dma', 'LDS-DMA loads'), ('waterfall', 'waterfall loops'),
            ('lds', 'LDS B'), ('insts', 'instructions')]
    print('| kernel | ' + ' | '.join(t for _, t in keys) + ' |\n|' + '---|' * (len(keys) + 1))
    for n in diff:
        print('| `%s` | ' % dem(n) + ' | '.join('%s → %s' % (ma[n].get(k, '?'), mb[n].get(k, '?')) for k, _ in keys) + ' |')
    diff = []
for n in diff:
    print('DIFFERS', dem(n))
for n in a:
    if n not in b:
        print('GONE', dem(n))
for n in b:
    if n not in a:
        print('NEW', dem(n), mb[n])
