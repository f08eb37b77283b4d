"""-m gpu: the drop-in `var` class on day files in the reference's format, against the NumPy restatement (tests/var_ref.py) driven
the same way."""
import io

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytest.importorskip('pandas')

import var_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
D_TOPICS, HD = 15, 16


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')


def _write_days(folder, days, first):
    """trend_distribution_day<N>.csv, 16 rows of d space-separated numbers (what var.read_data parses)."""
    folder.mkdir()
    for i, day in enumerate(days):
        np.savetxt(str(folder / ('trend_distribution_day%d.csv' % (first + i))), day, delimiter=' ', fmt='%.17g')
    return str(folder)


def _reference_text(per_day):
    """The sixteen np.savetxt lines of var.py:401-417 from per-day arrays [N, 4]."""
    f = io.BytesIO()
    n = per_day.shape[0]
    for q, name in enumerate(('l1_final', 'l1_mean', 'JSD_final', 'JSD_mean')):
        a = per_day[:, q]
        np.savetxt(f, np.array(['array_' + name]), fmt='%s')
        np.savetxt(f, np.array([np.mean(a)]), fmt='%.3e')
        np.savetxt(f, np.array([np.std(a)]), fmt='%.3e')
        np.savetxt(f, a.reshape(1, n), delimiter=',', fmt='%.3e')
    return f.getvalue().decode()


def test_train_forecast_and_evaluate_test(gpu, tmp_path, capsys):
    from discrete_mean_field_game_amd.var import var
    days = R.synthetic_days(8, HD, D_TOPICS, 41)
    train, test = _write_days(tmp_path / 'train', days[:6], 1), _write_days(tmp_path / 'test', days[6:], 7)
    exp = var(d=D_TOPICS)
    df_train, df_test = exp.read_data(train=train, train_start=1, train_end=6, test=test, test_start=7, test_end=8)
    assert df_train.shape == (96, 15) and df_test.shape == (32, 15)
    # (pandas' default float parser is not round-trip exact: the class fits what it read, so the restatement gets the same rows)
    read = np.concatenate([df_train.values, df_test.values]).reshape(8, HD, D_TOPICS)
    assert np.abs(read - days).max() <= 4 * R.U
    days = read
    res = exp.train(max_lag=3, df_train=exp.df_train, ridge=1e-2)
    assert res.k_ar == 3 and res.status == 0 and res.coefs.shape == (3, 15, 15)
    ref = R.model(days, range(6), [6, 7], 3, 1e-2, 0)
    assert np.linalg.norm(res.params - ref['coef']) <= 1e-9 * np.linalg.norm(ref['coef'])
    fut = exp.forecast(num_prior=3, steps=32, topic=0, plot=0)
    assert fut is exp.df_future and fut.shape == (32, 15)
    staged = R.model(days, range(6), [6, 7], 3, 1e-2, 0, B=res.params)
    Y, X = days[:6].reshape(96, 15), days[6:].reshape(32, 15)
    assert np.all(np.abs(fut.values - staged['future']) <= R.forecast_tolerance(Y, X, 3, 1e-2, 0, HD, res.params))
    out = tmp_path / 'test.csv'
    arrays = exp.evaluate_test(outfile=str(out))
    assert open(str(out)).read() == _reference_text(staged['per_day'])
    assert np.abs(arrays['JSD_mean'] - staged['per_day'][:, 3]).max() <= 1e-12
    # evaluate_train part 2 from the device, part 1 on the host
    l1_final, jsd_final, l1_mean, jsd_mean = exp.evaluate_train()
    assert abs(l1_mean - staged['insample'][0]) <= 1e-12 and abs(jsd_mean - staged['insample'][1]) <= 1e-12
    F, X = R.fitted(days[:6].reshape(96, 15), 3, res.params)
    assert abs(l1_final - np.abs(X - F).sum(axis=1)[HD - 1 - 3::HD].mean()) <= 1e-12
    # validation: the mean over the held-out days of the hourly mean JSD
    got = exp.validation(32, df_train, df_test)
    assert abs(got - staged['metrics'][6]) <= 1e-12
    # a forecast that the test set does not cover is not scored
    exp.forecast(num_prior=3, steps=16, plot=0)
    assert exp.evaluate_test(outfile=str(out)) is None and exp.df_future.shape == (16, 15)
    capsys.readouterr()


def test_cross_validation(gpu, tmp_path, capsys):
    from discrete_mean_field_game_amd.var import var
    days = R.synthetic_days(6, HD, D_TOPICS, 43)
    train = _write_days(tmp_path / 'train', days, 1)
    exp = var(d=D_TOPICS)
    exp.read_data(train=train, train_start=1, train_end=6, test=str(tmp_path / 'none'), test_start=1, test_end=0)
    assert len(exp.df_test) == 0 and np.abs(exp.df_train.values.reshape(6, HD, D_TOPICS) - days).max() <= 4 * R.U
    days = exp.df_train.values.reshape(6, HD, D_TOPICS).copy()
    out = tmp_path / 'cv.csv'
    lag_range = range(1, 6)
    best, errors = exp.cross_validation(lag_range, 2, 3, seed=5, outfile=str(out))
    # the restatement, driven by the same splits
    splits = var.splits(6, 2, 15, np.random.RandomState(5))
    want = []
    for i, lag in enumerate(lag_range):
        acc = 0
        for rep in range(3):
            sel, rest = splits[i * 3 + rep]
            k = i * 3 + rep
            B = exp.cv_fits.coef[k, :1 + lag * D_TOPICS]
            staged = R.model(days, sel, rest, lag, 1e-8, 0, B=B)
            tol = R.forecast_tolerance(R.series(days, sel), R.series(days, rest), lag, 1e-8, 0, HD, B)
            assert np.all(np.abs(exp.cv_fits.future[k, :32] - staged['future']) <= tol), (lag, rep)
            acc += R.metrics(exp.cv_fits.future[k, :32], R.series(days, rest), HD)[1][6]
        want.append(acc / 3)
    assert np.abs(np.array(errors) - np.array(want)).max() <= 1e-12
    assert best == list(lag_range)[int(np.argmin(want))]
    lines = open(str(out)).read().split('\n')
    assert lines[0] == '1,2,3,4,5' and lines[1] == ','.join(map(str, errors)) and lines[2:] == ['']
    assert len(errors) == 5 and all(np.isfinite(errors))
    capsys.readouterr()
