// Exercises the key-set members of include/barnett_smart.hpp -- key_set, key_set_update, key_set_clear, key_set_live, deal and
// verify_deal by index, seat and verify_shuffle_chains by index -- against the development emulator: three tables shuffled 2, 1 and 3 times under their own keys, the
// keys in slots 4, 0 and 2 of a set of five; the words by index are those of verify_shuffle_chains with the keys written out, a refused
// key and a cleared slot give MP_ERR_BAD_ARGUMENT on every link of their table and leave the other tables' words alone.
// usage: mirror_keyset ; prints "mirror_keyset ok"
#include <cstdio>

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
  std::swap(chains[0].proofs[1], chains[2].proofs[1]);      // one wrong link in the first and in the last table
  const std::vector<std::vector<int32_t>> want = cards.verify_shuffle_chains(pp, chains);
  if (want[0][0] != 0 || want[0][1] <= 0 || want[1][0] != 0 || want[2][1] <= 0) return fail("verify_shuffle_chains: the words with the keys written out");

  mp_keyset* ks = cards.key_set(pp, pl.keys[0], 5);
  if (cards.key_set_live(ks) != 0) return fail("a new set has live slots");
  const std::vector<uint32_t> slots = {4, 0, 2};
  if (cards.key_set_update(ks, slots, pl.keys) != std::vector<int32_t>(3, 0)) return fail("key_set_update: status words");
  if (cards.key_set_live(ks) != 3) return fail("three slots are live");
  if (cards.verify_shuffle_chains(pp, ks, slots, chains) != want) return fail("verify_shuffle_chains by index: the words differ");

  // dealing by index: the bytes and words of deal / verify_deal with the keys written out
  std::vector<uint32_t> slot_index;
  for (uint32_t k : key_index) slot_index.push_back(slots[k]);
  const DLCards::DealtCards by_index = cards.deal(deal_seeds, ks, slot_index, plain, factors);
  if (by_index.status != dealt.status || by_index.cards != dealt.cards || by_index.proofs != dealt.proofs) return fail("deal by index: bytes differ");
  if (cards.verify_deal(ks, slot_index, plain, dealt.cards, dealt.proofs) != std::vector<int32_t>(3 * N, 0)) return fail("verify_deal by index");
  // seating into the set: three tables of one player each, into slots 1, 3 and 2; the sums are the players' keys
  const DLCards::SeatedKeys seated = cards.seat(ks, {1, 3, 2}, {1, 1, 1}, pl.keys, pl.proofs, fs);
  if (seated.slot_status != std::vector<int32_t>(3, 0) || seated.sums.keys != pl.keys || cards.key_set_live(ks) != 5) return fail("seat: words or sums");
  if (cards.verify_shuffle_chains(pp, ks, {1, 3, 2}, chains) != want) return fail("verify_shuffle_chains under the seated slots");
  cards.key_set_clear(ks, {1, 3});

  bool threw = false;
  try {
    cards.key_set_update(ks, {1, 1}, {pl.keys[0], pl.keys[1]});
  } catch (const CardProtocolError&) {
    threw = true;
  }
  if (!threw || cards.key_set_live(ks) != 3) return fail("a slot named twice must be refused and change nothing");

  PublicKey identity{};
  if (cards.key_set_update(ks, {0}, {identity}) != std::vector<int32_t>(1, MP_ERR_BAD_ENCODING)) return fail("the identity must be refused");
  cards.key_set_clear(ks, {2});
  if (cards.key_set_live(ks) != 1) return fail("one slot is live after a refused key and a clear");
  const std::vector<std::vector<int32_t>> got = cards.verify_shuffle_chains(pp, ks, slots, chains);
  if (got[0] != want[0]) return fail("the table on the untouched slot: its words moved");
  if (got[1] != std::vector<int32_t>(1, MP_ERR_BAD_ARGUMENT) || got[2] != std::vector<int32_t>(3, MP_ERR_BAD_ARGUMENT))
    return fail("tables on empty slots: every link must read MP_ERR_BAD_ARGUMENT");
  cards.key_set_close(ks);
  std::printf("mirror_keyset ok\n");
  return 0;
}
