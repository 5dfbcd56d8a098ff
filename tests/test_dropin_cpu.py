"""The drop-in claim: reference-style drivers, launched through
tools/run_reference_driver.py, bind every detector-path name to THIS package, not to the
files that lie next to the driver.

Self-contained: the drivers are stand-ins written here into a scratch directory, laid out like
the reference's checkout (flat modules config / data / channel / loss / vamp / bamp / scamp /
plotter next to vamp_model.py, bamp_model.py and scamp_model.py, each driver importing its names
flat and defining its own Model).  With AMP_REFERENCE=<reference checkout> the reference's own
driver files are probed instead.  Nothing is executed on a device."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'amp-sparc-spatialmodulation_amd')

# driver file -> the names it imports from the modules this package replaces
DRIVERS = {
    'vamp_model.py': ('Config', 'Data', 'Channel', 'Loss', 'VAMP'),
    'bamp_model.py': ('Config', 'Data', 'Channel', 'Loss', 'BAMP'),
    'scamp_model.py': ('Config', 'Data', 'Channel', 'Loss', 'SCAMP'),
}
# the flat module every name comes from; plotter is the one module the package does not replace
MODULE_OF = {'Config': 'config', 'Data': 'data', 'Channel': 'channel', 'Loss': 'loss', 'VAMP': 'vamp',
             'BAMP': 'bamp', 'SCAMP': 'scamp', 'Plotter': 'plotter'}

PROBE = r'''
import json, sys, inspect
sys.dont_write_bytecode = True
sys.path.insert(0, {tools!r})
import run_reference_driver as rrd
mod = rrd.import_driver({driver!r})
out = {{}}
for name in {names!r}:
    obj = getattr(mod, name)
    out[name] = inspect.getsourcefile(obj)
out['Model'] = inspect.getsourcefile(mod.Model)
out['Plotter'] = inspect.getsourcefile(mod.Plotter)
print(json.dumps(out))
'''


@pytest.fixture(scope='module')
def ref_dir(tmp_path_factory):
    """The directory the drivers lie in: AMP_REFERENCE if given, else a stand-in checkout."""
    ref = os.environ.get('AMP_REFERENCE')
    if ref:
        assert os.path.isdir(ref), f'AMP_REFERENCE={ref} is not a directory'
        return ref
    d = tmp_path_factory.mktemp('standin_reference')
    for name, module in MODULE_OF.items():
        (d / f'{module}.py').write_text(f'class {name}:\n    """stand-in next to the driver"""\n')
    for driver, names in DRIVERS.items():
        lines = ['from torch import nn'] + [f'from {MODULE_OF[n]} import {n}' for n in names]
        lines += ['from plotter import Plotter', '', '', 'class Model(nn.Module):', '    pass', '', '',
                  "if __name__ == '__main__':", "    raise SystemExit('the probe imports the driver, it does not run it')"]
        (d / driver).write_text('\n'.join(lines) + '\n')
    return str(d)


@pytest.mark.parametrize('driver', sorted(DRIVERS))
def test_reference_driver_binds_package(driver, ref_dir):
    path = os.path.join(ref_dir, driver)
    assert os.path.exists(path), path
    if os.environ.get('AMP_REFERENCE'):
        pytest.importorskip('matplotlib')      # the reference's drivers import its plotter
    code = PROBE.format(tools=os.path.join(REPO, 'tools'), driver=path, names=DRIVERS[driver])
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    # run from another directory, the way the launcher is used (not from the driver's)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=REPO,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    files = json.loads(out.stdout.strip().splitlines()[-1])
    for name in DRIVERS[driver]:
        assert os.path.abspath(files[name]).startswith(PKG), (name, files[name])
    # the driver's own Model class stays the driver's (it is the code being dropped onto), and a
    # module the package does not replace still comes from the driver's directory
    assert os.path.abspath(files['Model']).startswith(os.path.abspath(ref_dir)), files['Model']
    assert os.path.abspath(files['Plotter']).startswith(os.path.abspath(ref_dir)), files['Plotter']


def test_plain_python_would_load_the_reference(ref_dir):
    """Why the launcher exists: `python driver.py` puts the driver's directory first, ahead of
    PYTHONPATH, so a flat `import vamp` there resolves to the file next to the driver."""
    code = 'import sys; sys.dont_write_bytecode = True; import vamp; print(vamp.__file__)'
    env = dict(os.environ, PYTHONPATH=PKG, PYTHONDONTWRITEBYTECODE='1')
    out = subprocess.run([sys.executable, '-c',
                          f'import sys; sys.path.insert(0, {ref_dir!r}); exec({code!r})'],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert os.path.abspath(out.stdout.strip()).startswith(os.path.abspath(ref_dir))
