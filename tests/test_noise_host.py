"""postprocess_influence_of_noise against what the reference's function wrote for the same table
(tests/golden/noise_stats.npz, tests/golden/generate_noise_golden.py), and the noise CLI's refusals
that need no device."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_stats.npz")


def test_postprocess_matches_the_reference(tmp_path):
    from annealing_sign_problem_amd.influence_of_noise import postprocess_influence_of_noise

    golden = np.load(GOLDEN)
    table, expected = golden["table"], golden["stats"]
    name = tmp_path / "noise.csv"
    with open(name, "w") as f:
        for row in table:
            f.write("{},{},{}\n".format(*row))
    returned = postprocess_influence_of_noise(str(name))
    with open(tmp_path / "noise_stats.csv") as f:
        assert f.readline() == "amplitude_overlap,median,upper,lower\n"
        written = np.loadtxt(f, delimiter=",")
    assert expected.shape == (100, 4)
    empty = np.isnan(expected[:, 1])
    assert 0 < empty.sum() < 100  # the table has empty bins and filled ones
    # the file holds the same numbers as the reference's (same text format), NaN where it has NaN
    np.testing.assert_array_equal(written, expected)
    np.testing.assert_array_equal(returned, written)


def test_cli_refuses_to_overwrite(tmp_path, capsys):
    from annealing_sign_problem_amd import influence_of_noise

    output = tmp_path / "noise.csv"
    output.write_text("kept\n")
    assert influence_of_noise.main(["--model", "heisenberg_kagome_16", "--seed", "1", "--output", str(output)]) == 1
    assert "not overwritten" in capsys.readouterr().err
    assert output.read_text() == "kept\n"


def test_postprocess_looks_only_at_rows_inside_a_bin(tmp_path):
    """A row whose amplitude overlap is exactly 0 falls in no bin (the bins are half-open from below):
    its sign overlap is not looked at.  Inside a bin a sign overlap above 1 is an error; a name without
    the .csv suffix is refused instead of being written over."""
    import pytest

    from annealing_sign_problem_amd.influence_of_noise import postprocess_influence_of_noise

    name = tmp_path / "noise.csv"
    name.write_text("1.0,0.0,1.5\n1.0,0.505,0.25\n1.0,0.505,0.75\n")
    stats = postprocess_influence_of_noise(str(name))
    assert np.isnan(stats[:, 1]).sum() == 99 and stats[50].tolist() == [0.505, 0.5, 0.625, 0.375]
    name.write_text("1.0,0.505,1.5\n")
    with pytest.raises(ValueError, match="above 1"):
        postprocess_influence_of_noise(str(name))
    plain = tmp_path / "noise.txt"
    plain.write_text("1.0,0.505,0.5\n")
    with pytest.raises(ValueError, match="csv"):
        postprocess_influence_of_noise(str(plain))
    assert plain.read_text() == "1.0,0.505,0.5\n"
