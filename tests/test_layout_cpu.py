"""The layout rule of tests/: no module imports a test module.  Helpers, case tables and constants that more than one file needs live
in the support and cases modules ("Where the tests' shared helpers live"), so a test module's import-time state -- its
parametrisation tables, module-level asserts and caches -- belongs to that module alone."""
import ast
import glob
import os

TESTS = os.path.dirname(os.path.abspath(__file__))


def _imported_test_modules(source):
    """(line, module) of every import of a test module of this package in a module's source, at any depth (function-level imports included)."""
    found = []
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Import):
            names = [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            base = '.' * node.level + (node.module or '')
            names = [base] + [f'{base}.{a.name}' for a in node.names]
        else:
            continue
        for name in names:
            parts = [p for p in name.split('.') if p]
            if name.startswith('.') or os.path.exists(os.path.join(TESTS, parts[0] + '.py')):      # relative, or found through tests/ on sys.path
                parts = ['tests'] + parts
            if parts[0] == 'tests' and any(p.startswith('test_') for p in parts[1:]):
                found.append((node.lineno, name))
                break
    return found


def test_no_module_under_tests_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(TESTS, '*.py')))
    assert len(files) > 40 and os.path.abspath(__file__) in files
    offenders = [f'{os.path.basename(path)}:{line} imports {name}' for path in files for line, name in _imported_test_modules(open(path).read())]
    assert not offenders, 'a test module is imported (move what is shared to a support or cases module): ' + '; '.join(offenders)
