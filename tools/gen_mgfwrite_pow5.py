"""Prints the power-of-five tables of `falcon_amd/csrc/numtext.h` (the block between its GENERATED markers), from exact integer
arithmetic.  The shortest-digits conversion of a float32 widened to double needs, with e2 the binary exponent of the double's
integer significand less 2 (-203 .. 73):
  kNumPow5Inv[q], q = 0 .. 21 : floor(2^(bitlength(5^q) - 1 + 125) / 5^q) + 1     (e2 >= 0: the value is divided by 10^q)
  kNumPow5[i],    i = 0 .. 63 : the top 125 bits of 5^i (shifted left below that)  (e2 <  0: the value is multiplied by 5^i)
each as {low 64 bits, high 64 bits}.  tests/test_mgfwrite_cpu.py checks the header's entries against the same expressions.

    python tools/gen_mgfwrite_pow5.py
"""
BITS = 125
N_INV, N_POW = 22, 64


def pow5_inv(q: int) -> int:
    p = 5 ** q
    return (1 << (p.bit_length() - 1 + BITS)) // p + 1


def pow5(i: int) -> int:
    p = 5 ** i
    shift = p.bit_length() - BITS
    return p >> shift if shift >= 0 else p << -shift


def _rows(name, values):
    out = [f"static constexpr uint64_t {name}[{len(values)}][2] = {{"]
    for v in values:
        assert v < 1 << 128
        out.append(f"    {{0x{v & (2 ** 64 - 1):016x}ull, 0x{v >> 64:016x}ull}},")
    out.append("};")
    return out


def main() -> None:
    lines = _rows("kNumPow5Inv", [pow5_inv(q) for q in range(N_INV)]) + _rows("kNumPow5", [pow5(i) for i in range(N_POW)])
    print("\n".join(lines))


if __name__ == "__main__":
    main()
