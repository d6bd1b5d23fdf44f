"""CPU: the whole ctypes mirror (nfmc_amd/abi.py) against include/nfmc_hip.h, in one place.  `mismatches` walks a
namespace: every Structure in it (size, every field's offset, size, name and place, from one C program compiled against
the header), the set of structs both ways, every NFMC_* word, DIAG_ROWS and RANK_SERIES, every prototype's restype and
argtypes, and the words that mirror constants of the kernels' sources.  A new struct, word or entry point is picked up
without a test of its own; the doctored namespaces below are what shows that the check bites."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from nfmc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nfmc_amd', 'csrc')
HEADER = open(os.path.join(ROOT, 'include', 'nfmc_hip.h')).read()

# header words that have no Python twin on purpose; every other NFMC_* word of the header must be mirrored
NOT_MIRRORED = {'NFMC_HIP_H',                                                   # the include guard
                'NFMC_DIAG_SUM_M', 'NFMC_DIAG_SUM_M2', 'NFMC_DIAG_SUM_MH', 'NFMC_DIAG_SUM_MH2', 'NFMC_DIAG_SUM_S2H',
                'NFMC_DIAG_SUM_MU', 'NFMC_DIAG_SUM_MU2', 'NFMC_DIAG_SUM_BT',    # the rows behind DIAG_ROWS, by position
                'NFMC_BLOB_MAX_PIECES', 'NFMC_PRP_ROUNDS'}                      # limits the host never needs
# words of the mirror that restate a constant of the kernels' sources: name -> (file of csrc, constant)
KERNEL_WORDS = {'TAG_NOISE': ('common.hpp', 'kTagNoise'), 'TAG_ACCEPT': ('common.hpp', 'kTagAccept'),
                'TAG_LATENT': ('common.hpp', 'kTagLatent'), 'TAG_JUMP': ('common.hpp', 'kTagJump'),
                'STAT_TAIL': ('common.hpp', 'kStatTail'), 'MIXTURE_MAX_COMPONENTS': ('pot_kinds.hpp', 'kMixMaxK'),
                'TAG_VELOCITY': None}   # exempt, no kernel constant: the mclmc driver passes it to nfmc_philox_normals_f32
SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'float': C.c_float,
           'nfmc_stream_t': C.c_void_p}


def header_structs(text):
    """{name: [field, ...]} of every `typedef struct { ... } Name;` of the comment-stripped header text."""
    out = {}
    for m in re.finditer(r'\}\s*(\w+)\s*;', text):
        start = text.rfind('typedef struct {', 0, m.start())
        body = text[start + len('typedef struct {'):m.start()]
        if start < 0 or '}' in body:
            continue
        out[m.group(1)] = [re.search(r'(\w+)\s*$', re.sub(r'\[[^\]]*\]', '', piece)).group(1)
                           for decl in body.split(';') if decl.strip() for piece in decl.split(',')]
    return out


def header_prototypes(text):
    """[(return type, name, [argument type, ...])] of every `ret name(args);`, the argument names dropped."""
    found = re.findall(r'(?m)^[ \t]*([A-Za-z_][\w \t\*]*?)\s*\b(nfmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    return [(ret, name, [] if args.strip() in ('', 'void') else [re.sub(r'\w+\s*$', '', a.strip()) for a in args.split(',')])
            for ret, name, args in found]


def bindings(ctype, structs):
    """The ctypes a C type may be bound as (compared by identity); () for a type outside the mapping."""
    ctype = re.sub(r'\bconst\b', '', ctype)
    base, stars = ' '.join(ctype.replace('*', ' ').split()), ctype.count('*')
    if stars != 1:
        return (SCALARS[base],) if stars == 0 and base in SCALARS else ()
    if base == 'char':
        return (C.c_char_p,)
    if base.startswith('Nfmc'):
        return (C.POINTER(structs[base]),) if base in structs else ()
    if base in ('int32_t', 'int64_t'):
        return (C.POINTER(SCALARS[base]), C.c_void_p)
    return (C.c_void_p,)


def evaluate(header_text, exprs):
    """The values of C integer expressions against the header text: one program, one gcc run."""
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, 'nfmc_hip.h'), 'w') as fh:
            fh.write(header_text)
        with open(os.path.join(td, 's.c'), 'w') as fh:
            fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "nfmc_hip.h"\nint main(void){\n'
                     + ''.join('printf("%%lld\\n", (long long)(%s));\n' % e for e in exprs) + 'return 0;}\n')
        exe = os.path.join(td, 's')
        subprocess.check_call(['gcc', '-I', td, os.path.join(td, 's.c'), '-o', exe])
        values = [int(v) for v in subprocess.check_output([exe]).split()]
    assert len(values) == len(exprs)
    return dict(zip(exprs, values))


def mismatches(namespace, header_text, partial=False):
    """Everything in which `namespace` (a dict: name -> object) is not a mirror of the header, one line per item, each
    naming the struct, field, word or prototype at fault; [] when it is one.  partial: the namespace mirrors some of
    the header's structs and nothing else (the stub of INTEGRATION.md): only those structs are held against it."""
    text = re.sub(r'/\*.*?\*/', ' ', header_text, flags=re.S)
    out = []
    structs = {k: v for k, v in namespace.items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    declared = header_structs(text)
    words = sorted(set(re.findall(r'\bNFMC_[A-Z0-9_]+\b', text)))
    ints = {k: v for k, v in namespace.items() if k.isupper() and isinstance(v, int) and not isinstance(v, bool)}
    twin = {w: 'NFMC_ABI_VERSION' if w == 'NFMC_ABI_VERSION' else w[len('NFMC_'):] for w in words}

    # ---- what the C program has to print: layouts of the structs both sides have, and the words
    want = {}
    for name, cls in structs.items():
        if name not in declared:
            out.append('%s: a struct of the mirror that the header does not declare' % name)
            continue
        fields = [f[0] for f in cls._fields_]
        if fields != declared[name]:
            out.append('%s: fields %s in the mirror, %s in the header' % (name, fields, declared[name]))
        want['sizeof(%s)' % name] = ('%s: size' % name, C.sizeof(cls))
        for f in fields:
            if f in declared[name]:
                want['offsetof(%s, %s)' % (name, f)] = ('%s.%s: offset' % (name, f), getattr(cls, f).offset)
                want['sizeof(((%s*)0)->%s)' % (name, f)] = ('%s.%s: size' % (name, f), getattr(cls, f).size)
    if not partial:
        out += ['%s: a struct of the header that the mirror lacks' % name for name in declared if name not in structs]
        for w in sorted(set(words) - NOT_MIRRORED):
            if twin[w] in ints:
                want[w] = ('%s: value' % twin[w], ints[twin[w]])
            else:
                out.append('%s: a word of the header with no int %s in the mirror' % (w, twin[w]))
    rows = [w for w in words if w.startswith('NFMC_DIAG_SUM_')]
    series = [w for w in words if w.startswith('NFMC_RANK_')]
    got = evaluate(header_text, list(want) + ([] if partial else rows + series))
    out += ['%s %d in the mirror, %d in the header' % (what, mine, got[e]) for e, (what, mine) in want.items() if mine != got[e]]
    if partial:
        return out

    # ---- words with no header twin, DIAG_ROWS, RANK_SERIES
    for k, where in KERNEL_WORDS.items():
        m = where and re.search(r'\b%s\s*=\s*(\d+)' % where[1], open(os.path.join(CSRC, where[0])).read())
        if where and (not m or int(m.group(1)) != ints.get(k)):
            out.append('%s: %s in the mirror, %s = %s in csrc/%s' % (k, ints.get(k), where[1], m and m.group(1), where[0]))
    out += ['%s: an int of the mirror that neither the header (NFMC_%s) nor a kernel constant stands behind' % (k, k)
            for k in ints if k not in twin.values() and k not in KERNEL_WORDS]
    by_position = [w[len('NFMC_DIAG_'):].lower() for w in sorted(rows, key=lambda w: got[w])]
    if sorted(got[w] for w in rows) != list(range(len(rows))) or tuple(by_position) != namespace.get('DIAG_ROWS'):
        out.append('DIAG_ROWS: %s in the mirror, %s in the header by position' % (namespace.get('DIAG_ROWS'), by_position))
    by_name = {w[len('NFMC_RANK_'):].lower(): got[w] for w in series}
    if by_name != namespace.get('RANK_SERIES'):
        out.append('RANK_SERIES: %s in the mirror, %s in the header' % (namespace.get('RANK_SERIES'), by_name))

    # ---- prototypes
    symbols = list(namespace.get('SYMBOLS', []))
    protos = header_prototypes(text)
    for names, where in (([s[0] for s in symbols], 'SYMBOLS'), ([p[1] for p in protos], 'the header')):
        out += ['%s: %d times in %s' % (n, names.count(n), where) for n in sorted(set(names)) if names.count(n) != 1]
    table = {s[0]: s for s in symbols}
    out += ['%s: in SYMBOLS, not declared in the header' % n for n in table if n not in {p[1] for p in protos}]
    for ret, name, args in protos:
        if name not in table:
            out.append('%s: declared in the header, not in SYMBOLS' % name)
            continue
        _, restype, argtypes = table[name]
        if not any(restype is t for t in bindings(ret, structs)):
            out.append('%s: restype %s for `%s`' % (name, getattr(restype, '__name__', restype), ret.strip()))
        if len(argtypes) != len(args):
            out.append('%s: %d argtypes for %d arguments' % (name, len(argtypes), len(args)))
            continue
        out += ['%s: argtypes[%d] is %s for `%s`' % (name, i, getattr(t, '__name__', t), a.strip())
                for i, (t, a) in enumerate(zip(argtypes, args)) if not any(t is b for b in bindings(a, structs))]
    return out


# ------------------------------------------------------------------------------------------------- the real mirror
def test_the_mirror_matches_the_header():
    assert mismatches(vars(abi), HEADER) == []


def test_the_parsers_see_the_whole_header_and_the_module_is_the_mirror_alone():
    text = re.sub(r'/\*.*?\*/', ' ', HEADER, flags=re.S)
    structs, protos = header_structs(text), header_prototypes(text)
    assert len(structs) == len(re.findall(r'typedef struct \{', text)) >= 28              # counted another way; no fewer than today
    assert len(protos) == len(set(re.findall(r'\b(nfmc_[a-z0-9_]+)\s*\(', text))) >= 57
    assert structs['NfmcAdamW'] == ['lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'step']          # comma-separated declarators
    assert structs['NfmcSelectArgs'][7:9] == ['carry', 'carry_prime']                                # array suffixes dropped
    assert ('const char*', 'nfmc_build_digest', []) in protos
    assert NOT_MIRRORED <= set(re.findall(r'\bNFMC_[A-Z0-9_]+\b', text))                             # no stale entry
    other = {k for k, v in vars(abi).items() if not k.startswith('__') and not isinstance(v, int)
             and not (isinstance(v, type) and issubclass(v, C.Structure))}
    assert other == {'C', 'c_fp', 'SYMBOLS', 'DIAG_ROWS', 'RANK_SERIES'}                             # ints, structs and these
    src = open(os.path.join(ROOT, 'nfmc_amd', 'abi.py')).read()
    assert re.findall(r'(?m)^\s*(?:import|from)\s+.*$', src) == ['import ctypes as C']
    from nfmc_amd import hip
    assert all(getattr(hip, k) is v for k, v in vars(abi).items() if not k.startswith('__'))       # hip.NAME for every name


# ------------------------------------------------------------------------------------------------- doctored mirrors
def doctored(**changes):
    """The mirror's namespace with `changes` put over it; a name given as None is removed."""
    return {k: v for k, v in dict(vars(abi), **changes).items() if v is not None}


def restruct(name, edit):
    """... with struct `name` rebuilt from its field list after `edit` changed it in place (SYMBOLS follows)."""
    old, fields = getattr(abi, name), list(getattr(abi, name)._fields_)
    edit(fields)
    new = type(name, (C.Structure,), {'_fields_': fields})
    rows = [(n, r, [C.POINTER(new) if t is C.POINTER(old) else t for t in a]) for n, r, a in abi.SYMBOLS]
    return doctored(SYMBOLS=rows, **{name: new})


def resymbol(name, restype=None, arg=None):
    """... with the row of `name` in SYMBOLS changed: its restype, or argtypes[arg[0]] = arg[1]."""
    rows = {s[0]: [s[1], list(s[2])] for s in abi.SYMBOLS}
    rows[name][0] = restype or rows[name][0]
    if arg:
        rows[name][1][arg[0]] = arg[1]
    return doctored(SYMBOLS=[(n, r, a) for n, (r, a) in rows.items()])


DOCTORED = [
    # two adjacent int32 fields swapped: the size stays, the offsets and the order do not
    ('swapped', lambda: restruct('NfmcTune', lambda f: f.insert(2, f.pop(3))),
     ['NfmcTune: fields', 'NfmcTune.tune_step_size: offset 20 in the mirror, 16', 'NfmcTune.tune_inv_mass_diag: offset 16 in the mirror, 20']),
    ('renamed', lambda: restruct('NfmcRng', lambda f: f.__setitem__(3, ('n_rounds', C.c_uint32))), ["NfmcRng: fields", "'n_rounds'"]),
    ('narrowed', lambda: restruct('NfmcFlowMhArgs', lambda f: f.__setitem__(2, ('n', C.c_int32))),
     ['NfmcFlowMhArgs.n: size 4 in the mirror, 8', 'NfmcFlowMhArgs.n_steps: offset 20 in the mirror, 24']),
    ('constant', lambda: doctored(TRAJ_CLIP=abi.TRAJ_CLIP + 1), ['TRAJ_CLIP: value 8 in the mirror, 7']),
    ('word_unmirrored', lambda: doctored(DIAG_MAX_LAG=None), ['NFMC_DIAG_MAX_LAG: a word of the header with no int DIAG_MAX_LAG']),
    ('word_of_nothing', lambda: doctored(POT_NEW=15), ['POT_NEW: an int of the mirror']),
    ('argtype', lambda: resymbol('nfmc_imh_parallel_work_bytes', arg=(0, C.c_int32)),
     ['nfmc_imh_parallel_work_bytes: argtypes[0] is c_int for `int64_t`']),
    ('argtype_struct', lambda: resymbol('nfmc_hmc_steps_f32', arg=(0, C.POINTER(abi.NfmcMalaArgs))),
     ['nfmc_hmc_steps_f32: argtypes[0] is LP_NfmcMalaArgs for `const NfmcHmcArgs*`']),
    ('restype', lambda: resymbol('nfmc_rows_sample_index', restype=C.c_int), ['nfmc_rows_sample_index: restype c_int for `int64_t`']),
    ('symbol_missing', lambda: doctored(SYMBOLS=abi.SYMBOLS[:-1]), ['nfmc_build_digest: declared in the header, not in SYMBOLS']),
    ('struct_removed', lambda: doctored(NfmcBlobPiece=None),
     ['NfmcBlobPiece: a struct of the header that the mirror lacks', 'nfmc_flow_blob_copy_f32: argtypes[1]']),
    ('diag_rows', lambda: doctored(DIAG_ROWS=abi.DIAG_ROWS[1::-1] + abi.DIAG_ROWS[2:]), ['DIAG_ROWS: ']),
    ('rank_series', lambda: doctored(RANK_SERIES=dict(abi.RANK_SERIES, folded=2, tail_low=1)), ['RANK_SERIES: ']),
    ('kernel_word', lambda: doctored(TAG_JUMP=4), ['TAG_JUMP: 4 in the mirror, kTagJump = 3 in csrc/common.hpp']),
]


@pytest.mark.parametrize('case', DOCTORED, ids=[c[0] for c in DOCTORED])
def test_a_doctored_mirror_is_named(case):
    """Every line names the doctored item, and every expected finding is among them."""
    _, doctor, expected = case
    found = mismatches(doctor(), HEADER)
    subjects = {e.split(':')[0].split('.')[0] for e in expected}
    assert found and all(line.split(':')[0].split('.')[0] in subjects for line in found), found
    assert all(any(e in line for line in found) for e in expected), found


def test_a_header_that_moved_on_is_named():
    """The other direction: the mirror as it is against a header with one more field, word, struct and entry point."""
    header = HEADER.replace('} NfmcLimits;', '    int32_t more;\n} NfmcLimits;\n#define NFMC_MORE 3\n'
                            'typedef struct {\n    int64_t n;\n} NfmcMore;\nint nfmc_more(const NfmcMore* m);')
    found = sorted(mismatches(vars(abi), header))
    want = ['NFMC_MORE: a word of the header', 'NfmcLimits: fields', 'NfmcLimits: size 24 in the mirror, 28',
            'NfmcMore: a struct of the header that the mirror lacks', 'nfmc_more: declared in the header, not in SYMBOLS']
    assert len(found) == len(want) and all(w in line for w, line in zip(want, found)), found


# ------------------------------------------------------------------------------------------------- literals
def test_pinned_values():
    """The literal values the per-feature tests used to pin, kept as literals: the checks above compare two texts, so
    an edit that changes both alike -- a renumbered kind, a field moved in the header and in the mirror -- shows here."""
    assert abi.NFMC_ABI_VERSION == 4
    kinds = ('QUADRATIC FUNNEL GAUSSIAN_MIXTURE LOGISTIC_REGRESSION GAUSSIAN_FULL ROSENBROCK STOCHASTIC_VOLATILITY '
             'SPARSE_LOGISTIC_REGRESSION LATTICE_PHI4 ITEM_RESPONSE VARYING_EFFECTS PARTICLES LATENT_GAUSSIAN LATENT_GMRF DIFFUSION_BRIDGE')
    assert [getattr(abi, 'POT_' + k) for k in kinds.split()] == list(range(15))
    assert abi.MIXTURE_MAX_COMPONENTS == 8
    assert [f[0] for f in abi.NfmcPotential._fields_][:2] == ['kind', 'n_components']
    assert C.sizeof(abi.NfmcTune) == 32 and abi.NfmcTune.trajectory.offset == 28
    assert abi.TRAJ_WORDS == 16
    assert abi.DIAG_MAX_LAG >= 127
    assert (abi.RANK_BULK, abi.RANK_FOLDED, abi.RANK_TAIL_LOW, abi.RANK_TAIL_HIGH) == (0, 1, 2, 3)
    assert abi.RANK_SERIES == {'bulk': 0, 'folded': 1, 'tail_low': 2, 'tail_high': 3}
    for cls, fields in ((abi.NfmcMclmcArgs, 'x velocity n d n_steps step_size decoherence_length inv_mass_diag pot rng stats samples '
                                            'energy_out energy_sums tune'),
                        (abi.NfmcMclmcTune, 'state inv_mass_diag tune_step_size tune_decoherence_length tune_inv_mass_diag every'),
                        (abi.NfmcNeutraMhArgs, 'z n n_steps adjust inv_mass_diag flow pot rng stats samples masks_out log_ratio_out')):
        assert [f[0] for f in cls._fields_] == fields.split(), cls
    rows = {s[0]: s[1:] for s in abi.SYMBOLS}
    assert rows['nfmc_mclmc_steps_f32'] == (C.c_int, [C.POINTER(abi.NfmcMclmcArgs), C.c_void_p])
    assert rows['nfmc_neutra_mh_steps_f32'] == (C.c_int, [C.POINTER(abi.NfmcNeutraMhArgs), C.c_void_p])
