// Exercises the ragged members of include/barnett_smart.hpp -- compute_reveal_tokens / open_cards with counts, compute_aggregate_keys with
// a count per table, verify_shuffle_chains -- against the library it is linked with (libmpshuffle.so on the GPU, the development emulator
// on the CPU).  Needs no case file: three tables of 2, 3 and 5 players are seated, dealt six cards each and shuffled 2, 1 and 3 times; every
// ragged member is held to its uniform twin on the items regrouped by count, and to the plaintexts that were dealt.
// usage: mirror_ragged ; prints "mirror_ragged ok"
#include <cstdio>
#include <cstring>

#include "barnett_smart.hpp"

using namespace barnett_smart;
typedef std::array<uint8_t, 32> Seed;

static Seed seed(uint8_t tag, size_t i) {
  Seed s{};
  s[0] = tag;
  s[1] = (uint8_t)i;
  s[2] = (uint8_t)(i >> 8);
  return s;
}
static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

int main() {
  const std::vector<uint32_t> seats = {2, 3, 5};
  const uint32_t m = 2, n = 3, N = m * n;
  DLCards cards(MP_CURVE_STARK, 0);
  const Parameters pp = cards.setup(seed(1, 0), m, n);

  // ---- seating
  std::vector<Seed> key_seeds, fs;
  for (size_t l = 0; l < 10; ++l) {
    key_seeds.push_back(seed(2, l));
    std::string info = "Key Ownership Proofplayer " + std::to_string(l);
    Seed d;
    mp_blake2s((const uint8_t*)info.data(), info.size(), d.data());
    fs.push_back(d);
  }
  const DLCards::PlayerKeys pl = cards.player_keygen_batch(key_seeds, pp, fs);
  const DLCards::AggregateKeys agg = cards.compute_aggregate_keys(pp, seats, pl.keys, pl.proofs, fs);
  if (agg.table_status != std::vector<int32_t>{0, 0, 0} || agg.player_status != std::vector<int32_t>(10, 0)) return fail("seating: status words");
  const size_t start[4] = {0, 2, 5, 10};
  for (size_t k = 0; k < 3; ++k) {      // the uniform member on one table at a time
    const std::vector<PublicKey> keys(pl.keys.begin() + start[k], pl.keys.begin() + start[k + 1]);
    const std::vector<DLCards::ZKProofKeyOwnership> proofs(pl.proofs.begin() + start[k], pl.proofs.begin() + start[k + 1]);
    const std::vector<Seed> f(fs.begin() + start[k], fs.begin() + start[k + 1]);
    const DLCards::AggregateKeys one = cards.compute_aggregate_keys(pp, (size_t)seats[k], keys, proofs, f);
    if (one.table_status[0] != 0 || one.keys[0] != agg.keys[k]) return fail("seating: the ragged and the uniform member differ");
  }
  {
    std::vector<DLCards::ZKProofKeyOwnership> bad = pl.proofs;
    bad[4] = pl.proofs[3];                // the last seat of table 1
    const DLCards::AggregateKeys a = cards.compute_aggregate_keys(pp, seats, pl.keys, bad, fs);
    if (a.table_status[0] != 0 || a.table_status[1] != 5 || a.table_status[2] != 0 || a.keys[0] != agg.keys[0] || a.keys[1] != PublicKey{} ||
        a.keys[2] != agg.keys[2])
      return fail("seating: a bad proof at the last seat of table 1");
    try {
      cards.compute_aggregate_keys(pp, std::vector<uint32_t>{2, 3, 4}, pl.keys, pl.proofs, fs);
      return fail("seating: counts that do not add up are accepted");
    } catch (const CardProtocolError&) {
    }
  }

  // ---- dealing: six cards per table (the plaintext points are the first six public keys)
  std::vector<PublicKey> plain;
  std::vector<uint32_t> key_index;
  std::vector<Seed> deal_seeds;
  std::vector<Scalar> factors;
  for (size_t k = 0; k < 3; ++k)
    for (size_t i = 0; i < N; ++i) {
      plain.push_back(pl.keys[i]);
      key_index.push_back((uint32_t)k);
      deal_seeds.push_back(seed(3, k * N + i));
      factors.push_back(seed(4, k * N + i));      // (any scalar below the group order)
      factors.back()[31] = 0;
    }
  const DLCards::DealtCards dealt = cards.deal(deal_seeds, pp, agg.keys, key_index, plain, factors);
  if (dealt.status != std::vector<int32_t>(3 * N, 0)) return fail("dealing: status words");

  // ---- the chains: 2, 1 and 3 links
  const uint32_t links[3] = {2, 1, 3};
  std::vector<DLCards::Chain> chains(3);
  for (size_t k = 0; k < 3; ++k) {
    chains[k].shared_key = agg.keys[k];
    chains[k].decks.push_back(std::vector<MaskedCard>(dealt.cards.begin() + k * N, dealt.cards.begin() + (k + 1) * N));
    for (uint32_t j = 0; j < links[k]; ++j) {
      const DLCards::SeededShuffles s = cards.shuffle_and_remask_batch_seeded({seed(5, 8 * k + j)}, pp, agg.keys[k], {chains[k].decks.back()});
      if (s.status[0] != 0) return fail("chains: a shuffle failed");
      chains[k].decks.push_back(s.decks[0]);
      chains[k].proofs.push_back(s.proofs[0]);
    }
  }
  std::vector<std::vector<int32_t>> st = cards.verify_shuffle_chains(pp, chains);
  if (st != std::vector<std::vector<int32_t>>{{0, 0}, {0}, {0, 0, 0}}) return fail("chains: honest chains");
  {
    std::vector<DLCards::Chain> bad = chains;
    bad[2].proofs[1] = chains[0].proofs[1];
    st = cards.verify_shuffle_chains(pp, bad);
    const std::vector<int32_t> one = cards.verify_shuffle_batch(pp, agg.keys[2], {bad[2].decks[1]}, {bad[2].decks[2]}, {bad[2].proofs[1]});
    if (st[0] != std::vector<int32_t>{0, 0} || st[1] != std::vector<int32_t>{0} || st[2] != std::vector<int32_t>{0, one[0], 0} || one[0] <= 0)
      return fail("chains: a swapped proof at link 1 of table 2");
    bad[1].proofs.clear();
    try {
      cards.verify_shuffle_chains(pp, bad);
      return fail("chains: a chain without links is accepted");
    } catch (const CardProtocolError&) {
    }
  }

  // ---- showdown: the first two cards of every table's last deck, one token per seated player
  std::vector<MaskedCard> shown;
  std::vector<uint32_t> counts, signer;
  for (size_t k = 0; k < 3; ++k)
    for (size_t i = 0; i < 2; ++i) {
      shown.push_back(chains[k].decks.back()[i]);
      counts.push_back(seats[k]);
      for (size_t j = start[k]; j < start[k + 1]; ++j) signer.push_back((uint32_t)j);
    }
  std::vector<Seed> token_seeds;
  for (size_t l = 0; l < signer.size(); ++l) token_seeds.push_back(seed(6, l));
  const PublicKey any = agg.keys[0];
  const DLCards::RevealedTokens rv = cards.compute_reveal_tokens(token_seeds, pp, any, pl.keys, pl.secret_keys, shown, signer, counts);
  if (rv.status != std::vector<int32_t>(signer.size(), 0)) return fail("showdown: reveal status words");
  const std::vector<PublicKey> card_list(plain.begin(), plain.begin() + N);
  const DLCards::OpenedCards op = cards.open_cards(pp, any, pl.keys, shown, signer, rv.tokens, rv.proofs, card_list, counts);
  if (op.card_status != std::vector<int32_t>(6, 0) || op.token_status != std::vector<int32_t>(signer.size(), 0)) return fail("showdown: open status words");
  for (size_t c = 0; c < 6; ++c)
    if (op.index[c] >= N || op.plaintexts[c] != card_list[op.index[c]]) return fail("showdown: a card does not open to a dealt card");
  for (size_t k = 0, lane = 0; k < 3; lane += 2 * seats[k], ++k) {      // the uniform members on the two cards of one table
    const std::vector<MaskedCard> two(shown.begin() + 2 * k, shown.begin() + 2 * k + 2);
    const std::vector<uint32_t> sg(signer.begin() + lane, signer.begin() + lane + 2 * seats[k]);
    const std::vector<Seed> sd(token_seeds.begin() + lane, token_seeds.begin() + lane + 2 * seats[k]);
    const DLCards::RevealedTokens u = cards.compute_reveal_tokens(sd, pp, any, pl.keys, pl.secret_keys, two, sg);
    if (!std::equal(u.tokens.begin(), u.tokens.end(), rv.tokens.begin() + lane) || !std::equal(u.proofs.begin(), u.proofs.end(), rv.proofs.begin() + lane))
      return fail("showdown: the ragged and the uniform compute_reveal_tokens differ");
    const DLCards::OpenedCards o = cards.open_cards(pp, any, pl.keys, two, sg, u.tokens, u.proofs, card_list);
    if (o.plaintexts[0] != op.plaintexts[2 * k] || o.plaintexts[1] != op.plaintexts[2 * k + 1] || o.index[0] != op.index[2 * k] ||
        o.index[1] != op.index[2 * k + 1])
      return fail("showdown: the ragged and the uniform open_cards differ");
  }
  {
    std::vector<DLCards::RevealToken> bad = rv.tokens;
    bad[2 * 2 + 2 * 3 - 1] = pl.keys[0];      // the last token of card 3: card 4's first one is the lane after it
    const DLCards::OpenedCards o = cards.open_cards(pp, any, pl.keys, shown, signer, bad, rv.proofs, card_list, counts);
    if (o.card_status != std::vector<int32_t>{0, 0, 0, 6, 0, 0} || o.plaintexts[4] != op.plaintexts[4] || o.index[3] != 0xFFFFFFFFu)
      return fail("showdown: a bad token at the last lane of card 3");
  }
  std::printf("mirror_ragged ok\n");
  return 0;
}
