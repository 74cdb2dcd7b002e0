"""The touched-key set's rule, key by key, in plain Python (hopscotch_hash_set.cc:104-122,173-195): an
insert that finds more than ``capacity`` keys drops the whole set first (dropped += size, clears += 1),
then adds the key if it is absent.  The device set must reach the same state for a whole batch taken in
order."""


class TruthSet:

  def __init__(self, capacity):
    self.capacity = int(capacity)
    self.keys = set()
    self.dropped = 0
    self.clears = 0

  def insert_one(self, fid, tag=0):
    if len(self.keys) > self.capacity:
      self.dropped += len(self.keys)
      self.clears += 1
      self.keys = set()
    self.keys.add((int(fid), int(tag)))

  def insert(self, ids, tag=0):
    """-> keys dropped by this call"""
    before = self.dropped
    for fid in ids:
      self.insert_one(fid, tag)
    return self.dropped - before

  def insert_segments(self, segments):
    """segments: [(ids, tag)] in segment-major, position-minor order"""
    before = self.dropped
    for ids, tag in segments:
      for fid in ids:
        self.insert_one(fid, tag)
    return self.dropped - before

  def steal(self):
    out = sorted(self.keys)
    self.keys = set()
    return out

  def stats(self):
    return (len(self.keys), self.dropped, self.clears, self.capacity)
