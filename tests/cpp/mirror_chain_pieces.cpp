// Exercises verify_shuffle_chains_dev and set_chain_pieces of include/barnett_smart.hpp against the development emulator, whose device
// pointers are host pointers: three tables shuffled 2, 1 and 3 times, their chains laid out table-major in plain vectors; both
// decompositions give the words of verify_shuffle_chains, for honest chains and with a proof swapped between tables.
// usage: mirror_chain_pieces ; prints "mirror_chain_pieces ok"
#include <cstdio>
#include <cstring>

#include "barnett_smart.hpp"

using namespace barnett_smart;
typedef std::array<uint8_t, 32> Seed;

static Seed seed(uint8_t tag, size_t i) {
  Seed s{};
  s[0] = tag;
  s[1] = (uint8_t)i;
  return s;
}
static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

int main() {
  const uint32_t m = 2, n = 3, N = m * n;
  DLCards cards(MP_CURVE_STARK, 0);
  const Parameters pp = cards.setup(seed(1, 0), m, n);
  std::vector<Seed> key_seeds, fs;
  for (size_t l = 0; l < 3; ++l) {
    key_seeds.push_back(seed(2, l));
    fs.push_back(seed(6, l));
  }
  const DLCards::PlayerKeys pl = cards.player_keygen_batch(key_seeds, pp, fs);
  std::vector<PublicKey> plain;
  std::vector<uint32_t> key_index;
  std::vector<Seed> deal_seeds;
  std::vector<Scalar> factors;
  for (size_t k = 0; k < 3; ++k)
    for (size_t i = 0; i < N; ++i) {
      plain.push_back(pl.keys[i % 3]);
      key_index.push_back((uint32_t)k);
      deal_seeds.push_back(seed(3, k * N + i));
      factors.push_back(seed(4, k * N + i));
      factors.back()[31] = 0;
    }
  const DLCards::DealtCards dealt = cards.deal(deal_seeds, pp, pl.keys, key_index, plain, factors);
  if (dealt.status != std::vector<int32_t>(3 * N, 0)) return fail("dealing: status words");
  const std::vector<uint32_t> links = {2, 1, 3};
  std::vector<DLCards::Chain> chains(3);
  for (size_t k = 0; k < 3; ++k) {
    chains[k].shared_key = pl.keys[k];
    chains[k].decks.push_back(std::vector<MaskedCard>(dealt.cards.begin() + k * N, dealt.cards.begin() + (k + 1) * N));
    for (uint32_t j = 0; j < links[k]; ++j) {
      const DLCards::SeededShuffles s = cards.shuffle_and_remask_batch_seeded({seed(5, 8 * k + j)}, pp, pl.keys[k], {chains[k].decks.back()});
      if (s.status[0] != 0) return fail("a shuffle failed");
      chains[k].decks.push_back(s.decks[0]);
      chains[k].proofs.push_back(s.proofs[0]);
    }
  }
  for (int swapped = 0; swapped < 2; ++swapped) {
    if (swapped) std::swap(chains[0].proofs[1], chains[2].proofs[1]);
    const std::vector<std::vector<int32_t>> want = cards.verify_shuffle_chains(pp, chains);
    std::vector<int32_t> flat;
    for (const std::vector<int32_t>& row : want) flat.insert(flat.end(), row.begin(), row.end());
    if (swapped ? (flat[0] != 0 || flat[1] <= 0 || flat[2] != 0 || flat[3] != 0 || flat[4] <= 0 || flat[5] != 0) : flat != std::vector<int32_t>(6, 0))
      return fail("verify_shuffle_chains: the words of the host-buffer member");
    // table-major: 16-byte aligned because every row is a multiple of 32 bytes and operator new aligns to 16
    std::vector<MaskedCard> decks;
    std::vector<PublicKey> keys;
    std::vector<uint8_t> pf;
    for (const DLCards::Chain& ch : chains) {
      for (const std::vector<MaskedCard>& d : ch.decks) decks.insert(decks.end(), d.begin(), d.end());
      for (const auto& p : ch.proofs) {
        pf.insert(pf.end(), p.begin(), p.end());
        keys.push_back(ch.shared_key);
      }
    }
    for (int mode : {MP_CHAIN_PIECES_WHOLE, MP_CHAIN_PIECES_BINARY}) {
      cards.set_chain_pieces(mode);
      std::vector<int32_t> st(6, 77);
      cards.verify_shuffle_chains_dev(pp, keys[0], links, keys[0].data(), decks[0].data(), pf.data(), st.data());
      cards.sync();
      if (st != flat) return fail("verify_shuffle_chains_dev differs from verify_shuffle_chains");
      uint64_t stats[8];
      if (mp_chain_ragged_stats(cards.table(), stats) != MP_OK || stats[0] != (mode ? 2u : 3u) || stats[1] != (mode ? 4u : 3u) || stats[5] != 0 ||
          stats[7] != (uint64_t)mode)
        return fail("mp_chain_ragged_stats after verify_shuffle_chains_dev");
    }
  }
  try {
    cards.set_chain_pieces(2);
    return fail("set_chain_pieces accepts mode 2");
  } catch (const CardProtocolError&) {
  }
  try {
    cards.verify_shuffle_chains_dev(pp, chains[0].shared_key, {}, nullptr, nullptr, nullptr, nullptr);
    return fail("verify_shuffle_chains_dev accepts no tables");
  } catch (const CardProtocolError&) {
  }
  std::printf("mirror_chain_pieces ok\n");
  return 0;
}
