"""CPU: the module layout of nfmc_amd/potentials/ (DESIGN.md "Module layout of the potential kinds"), the host-side
counterpart of test_host_include_structure.py.  Everything is read from the parsed sources: nothing is imported."""
import ast
import os

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nfmc_amd', 'potentials')

# module -> the classes it defines, and the hip.POT_* codes their descriptors carry
CLASSES = {
    '_base': ['Potential'],
    '_observations': ['SiteObservations'],
    'basic': ['QuadraticPotential', 'SumOfSquares', 'DiagonalGaussian', 'Funnel', 'GaussianMixture',
              'BayesianLogisticRegression'],
    'fullrank': ['FullRankGaussian'], 'rosenbrock': ['Rosenbrock'], 'sv': ['StochasticVolatility'],
    'slr': ['SparseLogisticRegression'], 'phi4': ['LatticePhi4'], 'irt': ['ItemResponseTheory'],
    'vfx': ['VaryingEffectsRegression'], 'particles': ['ParticleSystem'], 'lgm': ['LatentGaussianModel'],
    'gmrf': ['LatentGMRF'], 'diffusion': ['DiffusionBridge'], 'recognize': [],
}
CODES = {
    'basic': {'POT_QUADRATIC', 'POT_FUNNEL', 'POT_GAUSSIAN_MIXTURE', 'POT_LOGISTIC_REGRESSION'},
    'fullrank': {'POT_GAUSSIAN_FULL'}, 'rosenbrock': {'POT_ROSENBROCK'}, 'sv': {'POT_STOCHASTIC_VOLATILITY'},
    'slr': {'POT_SPARSE_LOGISTIC_REGRESSION'}, 'phi4': {'POT_LATTICE_PHI4'}, 'irt': {'POT_ITEM_RESPONSE'},
    'vfx': {'POT_VARYING_EFFECTS'}, 'particles': {'POT_PARTICLES'}, 'lgm': {'POT_LATENT_GAUSSIAN'},
    'gmrf': {'POT_LATENT_GMRF'}, 'diffusion': {'POT_DIFFUSION_BRIDGE'},
}
# what a module may import from the package besides _base (which imports nothing from it)
MAY_IMPORT = {'_base': set(), 'lgm': {'_observations'}, 'gmrf': {'_observations', 'lgm'}, 'diffusion': {'fullrank'},
              'recognize': {'basic'}}
PUBLIC = {'FAMILIES', 'Potential', 'recognize'} | {c for m, cs in CLASSES.items() if m != '_observations' for c in cs}


def parsed(module):
    with open(os.path.join(PKG, module + '.py')) as fh:
        return ast.parse(fh.read())


def package_imports(tree):
    """{module: names} of the `from .module import names` statements of a parsed module of the package."""
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            out.setdefault(node.module, set()).update(a.asname or a.name for a in node.names)
    return out


def test_the_table_names_every_module():
    assert sorted(list(CLASSES) + ['__init__']) == sorted(f[:-3] for f in os.listdir(PKG) if f.endswith('.py'))
    assert set(CODES) == set(CLASSES) - {'_base', '_observations', 'recognize'}


def test_the_package_exports_the_public_names_and_holds_no_code():
    tree = parsed('__init__')
    assert isinstance(tree.body[0], ast.Expr) and isinstance(tree.body[0].value.value, str)   # the docstring
    assert all(isinstance(node, ast.ImportFrom) and node.level == 1 for node in tree.body[1:])
    imports = package_imports(tree)
    names = sorted(n for ns in imports.values() for n in ns)
    assert len(names) == len(set(names))
    assert {n for n in names if not n.startswith('_')} == PUBLIC and len(PUBLIC) == 20
    # tests clear potentials._announced: the set recognize() itself uses
    assert [n for n in names if n.startswith('_')] == ['_announced'] and '_announced' in imports['recognize']
    for module, ns in imports.items():
        assert {n for n in ns if n in PUBLIC and n not in ('FAMILIES', 'recognize')} <= set(CLASSES[module]), module


def test_every_class_and_every_kind_code_has_one_module():
    kinds = set()
    for node in ast.walk(ast.parse(open(os.path.join(os.path.dirname(PKG), 'abi.py')).read())):
        if isinstance(node, ast.Assign):
            for target in node.targets:
                kinds |= {e.id for e in ast.walk(target) if isinstance(e, ast.Name) and e.id.startswith('POT_')}
    found = {}
    for module, classes in CLASSES.items():
        tree = parsed(module)
        assert [n.name for n in tree.body if isinstance(n, ast.ClassDef)] == classes, module
        found[module] = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith('POT_')}
    assert {m: c for m, c in found.items() if c} == CODES
    assert sorted(c for cs in CODES.values() for c in cs) == sorted(kinds) and len(kinds) == 15


def test_a_kind_module_imports_the_base_and_what_its_row_allows():
    for module in CLASSES:
        imports = package_imports(parsed(module))
        assert None not in imports, module                       # `from . import x` would go through __init__
        assert set(imports) - {'_base'} <= MAY_IMPORT.get(module, set()), module
        assert '_base' in imports or module == '_base', module
    assert '_design_and_labels' in package_imports(parsed('slr'))['_base']    # the (X, y) check lives in _base
