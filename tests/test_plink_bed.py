"""CPU: the PLINK .bed reader / writer (viprs_amd/io/plink_bed.py)."""
import numpy as np
import pytest

from viprs_amd.io.plink_bed import BED_MAGIC, pack_codes, read_bed, unpack_codes, write_bed


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17])
def test_round_trip(tmp_path, n):
    rng = np.random.default_rng(n)
    m = 7
    codes = rng.integers(0, 4, size=(m, n)).astype(np.uint8)
    bim = {"CHR": np.full(m, "22"), "SNP": np.array([f"rs{j}" for j in range(m)]), "POS": np.arange(m) * 10 + 5,
           "A1": np.array(list("ACGTACG")), "A2": np.array(list("CATGCAT"))}
    pheno = rng.normal(size=n)
    pheno[0] = np.nan
    prefix = str(tmp_path / "g")
    write_bed(prefix, codes, bim, pheno, trailing_bits=rng.integers(0, 256, size=m).astype(np.uint8))
    rows, n_read, table, ph = read_bed(prefix)
    assert n_read == n and rows.shape == (m, (n + 3) // 4) and rows.dtype == np.uint8
    assert np.array_equal(unpack_codes(rows, n), codes)
    for k in ("CHR", "SNP", "A1", "A2"):
        assert list(table[k]) == list(bim[k])
    assert np.array_equal(table["POS"], bim["POS"])
    assert np.isnan(ph[0]) and np.array_equal(ph[1:], pheno[1:])
    assert open(prefix + ".bed", "rb").read(3) == BED_MAGIC


def test_pack_is_the_documented_bit_layout():
    # sample i of a SNP: bits 2 (i % 4) .. 2 (i % 4) + 1 of byte i // 4
    codes = np.array([[0, 1, 2, 3, 3]], dtype=np.uint8)
    assert pack_codes(codes).tolist() == [[0b11100100, 0b00000011]]
    assert pack_codes(codes, trailing_bits=3).tolist() == [[0b11100100, 0b11111111]]
    assert np.array_equal(unpack_codes(pack_codes(codes, 3), 5), codes)


def test_refusals(tmp_path):
    codes = np.zeros((3, 5), dtype=np.uint8)
    prefix = str(tmp_path / "g")
    write_bed(prefix, codes)
    raw = open(prefix + ".bed", "rb").read()
    open(prefix + ".bed", "wb").write(bytes([0x6C, 0x1B, 0x00]) + raw[3:])
    with pytest.raises(ValueError, match="sample-major"):
        read_bed(prefix)
    open(prefix + ".bed", "wb").write(bytes([0x6C, 0x1C, 0x01]) + raw[3:])
    with pytest.raises(ValueError, match="magic"):
        read_bed(prefix)
    open(prefix + ".bed", "wb").write(raw + b"\0")
    with pytest.raises(ValueError, match="bytes"):
        read_bed(prefix)
    open(prefix + ".bed", "wb").write(raw[:-1])
    with pytest.raises(ValueError, match="bytes"):
        read_bed(prefix)
    with pytest.raises(ValueError):
        pack_codes(np.array([[4]]))
